// lmx_particles.h — device layout and launchers of the particle kernels (particle_kernels.hip), shared with lmx_capi_particles.hip.
//
// Every emitter of every registered system has one ParticleEmitterDev. Its channels lie back to back in one float buffer, `stride`
// floats apart: `capacity` slots (a multiple of four) and a guard the kernels never write. Particle counts live on the device
// (ParticleStateDev) and never travel to the host inside a step: grids are sized by reserved capacity, and a block whose chunk starts
// at or past the count exits after one load.
#pragma once

#include "lmx_kernels.h"
#include "lmx_particle_program.h"
#include "lumix_mi355.h"

namespace lmx {

constexpr uint32_t PARTICLE_BLOCK = PARTICLE_CHUNK;     // one lane per particle of a chunk
constexpr uint32_t PARTICLE_EMIT_BLOCK = 256;           // one lane per new particle
constexpr uint32_t PARTICLE_GUARD_FLOATS = 64;          // behind every channel and behind the frame buffer
constexpr uint32_t PARTICLE_SCAN_BLOCK = 1024;

struct ParticleEmitterDev {
	uint32_t system, prog_update, prog_emit, prog_output; // absolute record indices
	uint32_t channels, registers, outputs, emit_inputs;
	uint32_t capacity, stride, max_chunks, shadow_mask;
	uint64_t channel_base;  // float index of channel 0, slot 0
	uint32_t kill_base;     // first of max_chunks kill counters; the compaction's copy list starts at the same index
	uint32_t local;         // index within its system: emitter k's sub-emission is drained before emitter k + 1 updates
	uint32_t first_of_system; // global index of the system's emitter 0 (EMIT targets are system-local)
	uint32_t init_emit_count;
	uint32_t n_emit;        // EMIT instructions of the update program; 0: no staging
	uint32_t job_base;      // first of capacity x n_emit sub-emission jobs
	uint64_t stage_base;    // word index of the staging records [slot][n_emit] of PARTICLE_STAGE_WORDS words
	uint8_t emit_group[PARTICLE_MAX_EMITS];
	// A ribbon emitter: capacity = max_ribbons rings of ribbon_len slots, ring p of channel c at c * stride + p * ribbon_len
	uint32_t ribbon_len;    // max_ribbon_length, a multiple of four, <= 1024; 0: not a ribbon emitter
	uint32_t max_ribbons;
	uint32_t ribbon_base;   // first of max_ribbons ParticleRibbonDev records
	uint32_t ribbon_ord;    // index among the ribbon emitters (ParticleRibbonCount)
};

// One live ribbon, by its index in Emitter::ribbons. The ring map: a ribbon keeps its physical ring for life, so killRibbon moves no bytes.
struct ParticleRibbonDev {
	uint32_t ring;          // physical ring of the emitter's channels
	uint32_t length;
	uint32_t row;           // first row of the packed slice: the lengths of the ribbons before it
	uint32_t pad;
};

struct ParticleRibbonCount { // per ribbon emitter
	uint32_t emitter, n_ribbons, total, pad; // total: the sum of the lengths = Emitter::particles_count
};

// One call of ParticleSystem::emitRibbonPoints. Its lanes are [first_lane, first_lane + min(count, ribbon_len)): one per ring slot that is hit
struct ParticleRibbonJob {
	uint32_t emitter, ribbon, ring;
	uint32_t offset0, length0, emit_index0; // the ribbon before the call
	uint32_t count, first_lane;
	float total_time, time_step;
};

struct ParticleSystemDev {
	float values[8];        // ParticleSystemValues of the step (EMIT_INDEX is per particle and lives elsewhere)
	uint32_t globals_at, n_globals, pad[2];
};

// What MESH and SPLINE read for the particles of one system: its entity's mesh 0, pose and spline. Uniform over a block.
constexpr uint32_t PARTICLE_NO_SOURCE = 0xffffffffu;
constexpr uint32_t PARTICLE_SOURCE_BONES = 1u; // flags: the model has bones
struct ParticleSourceDev {
	uint32_t mesh_at;       // first vertex in mesh_positions (x 3 floats)
	uint32_t n_verts;       // 0: no model instance, model not ready or no mesh - the run ends at a MESH
	uint32_t skin_at;       // first LmxSkin in mesh_skins; PARTICLE_NO_SOURCE: the mesh has none
	uint32_t palette_at;    // first bone of the instance's palette; PARTICLE_NO_SOURCE: no pose
	uint32_t n_bones;
	uint32_t flags;
	uint32_t spline_at;     // first point in spline_points (x 3 floats)
	uint32_t n_points;      // 0: no spline component; otherwise >= 3
};

struct ParticleStateDev {   // per emitter
	uint32_t count, emit_index, overflow, killed;
};

struct ParticleEmitJob {    // one call of ParticleSystem::emit
	uint32_t emitter, count;
	float total_time, time_step; // TOTAL_TIME of the first new particle, and what each further one adds
};

struct ParticleCopyOp { uint32_t dst, src, len, pad; };

// One EMIT a particle executed: {1, target, 16 emit outputs}, at [slot * n_emit + ordinal] of the emitter's staging area
constexpr uint32_t PARTICLE_STAGE_WORDS = 18;
constexpr uint32_t PARTICLE_SUB_BLOCKS = 32; // blocks per emitter of the sub-emission launch: each strides over the emitter's jobs
// One drained record: ParticleSystem::emit(target, outputs, init_emit_count, 0), with the slots it got
struct ParticleSubJob { uint32_t stage_index, target, slot, emit_index, n; };

struct ParticlesDevice {
	const ParticleEmitterDev* emitters;
	const ParticleSystemDev* systems;
	const ParticleRec* prog;
	const ParticleGradient* gradients;
	const float* globals;
	float* channels;
	ParticleStateDev* state;
	uint32_t* kill;          // per chunk
	ParticleCopyOp* ops;     // per chunk
	uint32_t* n_ops;         // per emitter
	uint32_t* stage;         // staging records of the emitters whose update programs hold EMIT
	ParticleSubJob* sub_jobs;
	uint32_t* n_sub;         // per emitter: jobs of the last plan
	LmxParticleSlice* slices;
	float* frame;
	uint32_t n_emitters, seed, step, frame_floats;
	uint32_t level;          // only emitters with this index in their system take part; 0xffffffff: all
	const ParticleRibbonDev* ribbons;         // the live ribbons of every ribbon emitter, as the host's last call left them
	const ParticleRibbonCount* ribbon_counts; // per ribbon emitter
	uint32_t n_ribbon_emitters;
	const ParticleSourceDev* sources;         // per system
	const float* mesh_positions;
	const LmxSkin* mesh_skins;
	const float4* palette;                    // of the last lmx_skin_run (skin_kernels.hip "Palette layout")
	const float* spline_points;
};

size_t particle_chunk_lds_bytes(uint32_t registers, uint32_t shadow_channels);

hipError_t launch_particles_emit(hipStream_t s, const ParticlesDevice& d, const ParticleEmitJob* jobs, uint32_t n_jobs, uint32_t max_count);
// processChunk over every chunk of every emitter with the update program, then the compaction plan and its copies
// ... and, with `sub_emit`, the drain of the EMIT records into their targets behind them
hipError_t launch_particles_update(hipStream_t s, const ParticlesDevice& d, uint32_t max_chunks, uint32_t max_registers, uint32_t max_shadow, bool sub_emit);
// slice offsets, then processChunk with the output program
hipError_t launch_particles_fill(hipStream_t s, const ParticlesDevice& d, uint32_t max_chunks, uint32_t max_registers);

// Ribbon emitters (particle_kernels.hip, k_particles_ribbon_*). `max_groups`: the largest number of 1024-lane blocks one ribbon emitter needs,
// each holding floor(1024 / ribbon_len) whole ribbons.
// emitRibbonPoints of every job: total_lanes = the sum of min(count, ribbon_len) over the jobs
hipError_t launch_particles_ribbon_emit(hipStream_t s, const ParticlesDevice& d, const ParticleRibbonJob* jobs, uint32_t n_jobs, uint32_t total_lanes);
// Emitter::particles_count of every ribbon emitter into the state records
hipError_t launch_particles_ribbon_commit(hipStream_t s, const ParticlesDevice& d);
// the update program over ring slots [0, length) of every ribbon (updateRibbons' chunk loop)
hipError_t launch_particles_ribbon_update(hipStream_t s, const ParticlesDevice& d, uint32_t max_groups, uint32_t max_registers);
// the output program into the packed rows of every ribbon; behind launch_particles_fill, which lays out the slices
hipError_t launch_particles_ribbon_fill(hipStream_t s, const ParticlesDevice& d, uint32_t max_groups, uint32_t max_registers);

} // namespace lmx
