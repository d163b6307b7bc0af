// lmx_particle_program.h — the particle VM's program as the kernels of particle_kernels.hip read it: fixed-width records decoded and
// validated ONCE on the host (lmx_particle_program.cpp, plain C++) from the byte stream of ParticleSystemResource::Emitter::instructions
// (renderer/particle_system.h:72-122). The device parses no unaligned bytes, and no record can name memory outside an emitter's buffers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace lmx {

// ParticleSystemResource::InstructionType, in the engine's order
enum ParticleOp : uint8_t {
	P_END, P_ADD, P_COS, P_SIN, P_NOISE, P_SUB, P_EMIT, P_MUL, P_MULTIPLY_ADD, P_LT, P_MOV, P_RAND, P_KILL, P_SQRT, P_GT, P_MIX, P_GRADIENT, P_DIV,
	P_SPLINE, P_MESH, P_MOD, P_OR, P_AND, P_NOT, P_BLEND, P_MAX, P_MIN, P_CMP, P_CMP_ELSE, P_OP_COUNT
};
// ParticleSystemResource::DataStream::Type
enum ParticleStream : uint8_t { PS_NONE, PS_CHANNEL, PS_SYSTEM_VALUE, PS_OUT, PS_REGISTER, PS_LITERAL, PS_GLOBAL, PS_ERROR };
// ParticleSystemValues
enum ParticleSysValue : uint8_t { PSV_TIME_DELTA, PSV_TOTAL_TIME, PSV_EMIT_INDEX, PSV_RIBBON_INDEX, PSV_ENTITY_X, PSV_ENTITY_Y, PSV_ENTITY_Z, PSV_COUNT };

constexpr uint32_t PARTICLE_MAX_CHANNELS = 16, PARTICLE_MAX_REGISTERS = 16, PARTICLE_MAX_NESTING = 4, PARTICLE_MAX_GRADIENT = 8;
constexpr uint32_t PARTICLE_MAX_EMITS = 8;    // EMIT instructions per update program (each owns a staging record per particle)
constexpr uint32_t PARTICLE_CHUNK = 1024; // ParticleSystem::update's chunk (particle_system.cpp:1504)

struct ParticleOperand {
	uint8_t type, index;
	uint16_t pad;
	float value;
};

// what an END record does to the lane that reaches it (the scalar interpreter's end_counter / skip_stack, resolved at decode time)
enum ParticleEndKind : uint8_t { PE_RETURN, PE_CONTINUE, PE_JUMP, PE_EMIT_END /* closes an EMIT's block: outputs go where they went before */ };

struct ParticleRec {
	uint8_t op;
	uint8_t kind;   // END: ParticleEndKind
	uint16_t wmask; // whole-chunk CMP / CMP_ELSE: the channels its blocks write, when one of them can kill (0 otherwise)
	uint32_t a;     // CMP / CMP_ELSE: the record behind the true block; END of kind PE_JUMP: the target; GRADIENT: its table; RAND: its ordinal; EMIT: the target emitter;
	                // MESH: its ordinal among the program's MESH instructions (the draw's key)
	uint32_t b;     // whole-chunk CMP / CMP_ELSE: bit 0 = a block holds a KILL; EMIT: its ordinal among the program's EMITs; MESH / SPLINE: subindex (0..2)
	uint32_t c;     // whole-chunk CMP / CMP_ELSE: the next whole-chunk record
	ParticleOperand o[4]; // dst, op0, op1, op2 (RAND: o[1].value = from, o[2].value = to; CMP: o[0] = the condition; MESH: o[1] = the index, read and written)
};
static_assert(sizeof(ParticleRec) == 48, "read by the kernels sixteen bytes at a time");

struct ParticleGradient {
	uint32_t count, pad[3];
	float keys[8], values[8], ms[8]; // ms as processChunk computes them (particle_system.cpp:1230-1233)
};

// The byte stream and what belongs to it, as lmx_particles_set_program receives them.
struct ParticleProgramDesc {
	const uint8_t* bytes;
	uint32_t size, emit_offset, output_offset;
	uint32_t channels_count, registers_count, outputs_count, emit_inputs_count;
	uint32_t n_emitters; // of the system: EMIT targets are checked against it
	uint32_t n_globals;
	// What the system has declared (lmx_particles_set_mesh_source / lmx_particles_set_spline, a "none" declaration included). Decoding
	// stops at the first MESH / SPLINE whose source is not declared, with has_mesh_or_spline set: the caller refuses such a program.
	uint32_t sources;
};
constexpr uint32_t PARTICLE_SRC_MESH = 1u, PARTICLE_SRC_SPLINE = 2u;

struct ParticleProgram {
	std::vector<ParticleRec> recs; // update | emit | output sections back to back
	std::vector<ParticleGradient> gradients;
	uint32_t update_at = 0, emit_at = 0, output_at = 0;
	uint32_t rand_count = 0;
	uint16_t shadow_mask = 0; // union of the wmasks: channels that need a snapshot while a killing block runs
	uint32_t emit_count = 0;                      // EMIT instructions of the update program
	uint8_t emit_group[PARTICLE_MAX_EMITS] = {};   // the whole-chunk conditional each sits in, counted from 0: records are drained block by block
	uint32_t emit_target[PARTICLE_MAX_EMITS] = {}; // ... and the emitter of its system it emits into
	bool has_emit = false, has_mesh_or_spline = false;
	bool has_mesh = false, has_spline = false;
	bool stopped = false;                         // decoding ended at a MESH / SPLINE without a declared source: `recs` is a prefix
	uint32_t mesh_count = 0;                      // MESH instructions, numbered by byte offset
	bool has_kill = false;                        // a KILL anywhere in the update program (refused for ribbon emitters)
};

enum ParticleDecodeResult { PD_OK = 0, PD_INVALID = 1, PD_UNSUPPORTED = 2 /* well formed, but a form of MESH / SPLINE the device does not run */ };

// Decodes and validates. On PD_INVALID / PD_UNSUPPORTED `error` says what was wrong; `out` is then unspecified. Never reads outside [bytes, bytes + size).
ParticleDecodeResult particle_program_decode(const ParticleProgramDesc& desc, ParticleProgram& out, std::string& error);

} // namespace lmx
