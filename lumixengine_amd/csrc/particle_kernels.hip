// particle_kernels.hip — ParticleSystem::update and Emitter::fillInstanceData on the device (renderer/particle_system.cpp), for every
// emitter of every registered system in a fixed number of launches per step.
//
//   k_particles_emit     ParticleSystem::emit (:411-452): one lane per new particle runs the emit program through the scalar interpreter.
//   k_particles_commit   adds what was emitted to the device-resident counts (clamped to the reserved capacity: overflow bit).
//   k_particles_chunk    processChunk (:1052-1375): one block per 1024-particle chunk, one lane per particle. The whole-chunk instructions
//                        run per lane; CMP / CMP_ELSE blocks run per particle with the scalar interpreter's semantics (run, :684-1013) and
//                        their kills land as the reference's sequential swap-with-last does. <false>: update program, <true>: output program.
//   k_particles_plan     the head / tail compaction plan over the chunks' kill counts (:1518-1556): integer logic, one lane per emitter.
//   k_particles_compact  the plan's copies: parallel over every channel.
//   k_particles_subemit  sub-emission: the EMIT records a step staged, drained by k_particles_plan in the reference's order, run the target's emit program.
//   k_particles_slices   the frame's slice offsets: a scan over ((count + 3) & ~3) * outputs_count * 4 bytes.
//
// The decoded program (lmx_particle_program.h) is wave-uniform outside conditional blocks: `ip` is a loop counter there and the records
// come through scalar loads (the program is a kernel argument of its own, const and __restrict__: no store of the kernel can clobber it). The VM's registers are LDS pages of 1024 floats, indexed by lane (chunk-local: DESIGN §4.15 deviation 3).
// Arithmetic is fp32 under -ffp-contract=off; MULTIPLY_ADD is a multiply and an add, MIX is a + (b - a) * c.
// MESH and SPLINE read the tables of the lane's system (ParticleSourceDev: its entity's mesh 0, the palette of its pose, its spline).
#include "lmx_particles.h"
#include "lmx_skin_eval.h"

namespace lmx {

namespace {

constexpr uint32_t MAP_PRE = 0x8000u; // s_map: the slot's content is the origin's value from BEFORE the block ran (the snapshot)

__device__ __forceinline__ float bits_f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t f_bits(float f) { return __float_as_uint(f); }

// The reference's arithmetic is x86 SSE: an operation without a NaN operand that has no value (0 / 0, inf - inf, sqrt(-1), fmod(x, 0))
// gives the negative default NaN 0xffc00000, and a NaN operand comes back quieted, the first one first. The VM's results are compared
// bit for bit and feed sign-bit masks, so NaN results are put into that form (a compare and, on the rare path, two selects).
__device__ __forceinline__ float nan_x86(float r, float a, float b) {
	if (r != r) r = a != a ? bits_f(f_bits(a) | 0x00400000u) : b != b ? bits_f(f_bits(b) | 0x00400000u) : bits_f(0xffc00000u);
	return r;
}
__device__ __forceinline__ float f_add(float a, float b) { return nan_x86(a + b, a, b); }
__device__ __forceinline__ float f_sub(float a, float b) { return nan_x86(a - b, a, b); }
__device__ __forceinline__ float f_mul(float a, float b) { return nan_x86(a * b, a, b); }
__device__ __forceinline__ float f_div(float a, float b) { return nan_x86(a / b, a, b); }
__device__ __forceinline__ float f_sqrt(float a) { return nan_x86(sqrtf(a), a, a); }
#ifndef LMX_PARTICLE_NO_LIBM
__device__ __forceinline__ float f_mod(float a, float b) { return nan_x86(fmodf(a, b), a, b); }
__device__ __forceinline__ float f_sin(float a) { return nan_x86(sinf(a), a, a); }
__device__ __forceinline__ float f_cos(float a) { return nan_x86(cosf(a), a, a); }
#else // tests/test_isa_particle_kernels.py alone defines it (no build of the library does): without the library's fmod, sine and cosine expansions no fused multiply-add may be left
__device__ __forceinline__ float f_mod(float a, float b) { return a - b; }
__device__ __forceinline__ float f_sin(float a) { return a; }
__device__ __forceinline__ float f_cos(float a) { return -a; }
#endif

// hash / gnoise of particle_system.cpp:320-338. u32(floor(p)) is x86-64's: through a signed 64-bit conversion, low word kept, 0 out of range.
__device__ __forceinline__ float p_hash(uint32_t n) {
	n = (n << 13U) ^ n;
	n = n * (n * n * 15731U + 789221U) + 1376312589U;
	return float(n & 0x0fffffffU) / 268435456.0f; // float(0x0ffFFffF) rounds to 2^28
}
__device__ __forceinline__ float p_gnoise(float p) {
	const float fl = floorf(p);
	uint32_t i = 0;
	if (fabsf(fl) < 9223372036854775808.0f) i = (uint32_t)(uint64_t)(int64_t)fl;
	const float f = f_sub(p, float(i));
	const float u = f_mul(f_mul(f_mul(f, f), f), f_add(f_mul(f, f_sub(f_mul(f, 6.f), 15.f)), 10.f));
	const float v0 = p_hash(i + 0u);
	const float v1 = p_hash(i + 1u);
	return f_mul(f_sub(f_add(f_mul(v0, f_sub(1.f, u)), f_mul(v1, u)), 0.5f), 4.8f);
}

__device__ __forceinline__ uint32_t p_mix(uint32_t x) {
	x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
	return x;
}
// RAND: a counter-based draw keyed by (seed, emitter, step, particle, instruction ordinal) through RandomGenerator::randFloat's formula
__device__ __forceinline__ uint32_t p_draw(uint32_t seed, uint32_t emitter, uint32_t step, uint32_t particle, uint32_t ordinal) {
	uint32_t r = p_mix(seed ^ 0x9e3779b9u);
	r = p_mix(r ^ emitter);
	r = p_mix(r ^ step);
	r = p_mix(r ^ particle);
	return p_mix(r ^ ordinal);
}
__device__ __forceinline__ float p_rand(uint32_t seed, uint32_t emitter, uint32_t step, uint32_t particle, uint32_t ordinal, float from, float to) {
	const uint32_t r = p_draw(seed, emitter, step, particle, ordinal);
	return from + float((to - from) * (r * 2.328306435996595e-10));
}
constexpr uint32_t MESH_DRAW_DOMAIN = 0x80000000u; // MESH ordinals are keyed apart from RAND's: neither numbering moves the other's draws

// u32(x) of a float as x86-64 converts it: through a signed 64-bit conversion, low word kept; NaN and out of range give 0
__device__ __forceinline__ uint32_t u32_x86(float v) {
	uint32_t i = 0;
	if (fabsf(v) < 9223372036854775808.0f) i = (uint32_t)(uint64_t)(int64_t)v;
	return i;
}

// What one lane of the VM sees
struct Lane {
	float* ch;            // channel 0, slot 0 of the emitter
	uint32_t stride, slot;
	uint32_t rslot;       // the particle slot RAND is keyed by: `slot`, or ribbon x ribbon_len + ring slot where `ch` is a ribbon's ring
	float ribbon_index;   // RIBBON_INDEX: the lane's own ribbon; 0 outside ribbon emitters
	float* regs;          // LDS register pages
	uint32_t rstride, lane;
	const float* sysv;
	const float* globals;
	float* outp;          // the particle's output row (output program only)
	float total_time, emit_index; // the emit program's own TOTAL_TIME / EMIT_INDEX
	bool emitting;
	uint32_t seed, emitter, step;
	uint32_t* stage;      // the emitter's staging records (update program with EMIT only)
	uint32_t n_emit;
	const ParticlesDevice* dev; // MESH / SPLINE: the source tables, read where such an instruction runs
	uint32_t system;
};

__device__ __forceinline__ float lane_read(const Lane& L, const ParticleOperand& o) {
	switch (o.type) {
		case PS_CHANNEL: return L.ch[(size_t)o.index * L.stride + L.slot];
		case PS_REGISTER: return L.regs[o.index * L.rstride + L.lane];
		case PS_SYSTEM_VALUE:
			if (L.emitting && o.index == PSV_TOTAL_TIME) return L.total_time;
			if (o.index == PSV_EMIT_INDEX) return L.emit_index;
			if (o.index == PSV_RIBBON_INDEX) return L.ribbon_index;
			return L.sysv[o.index];
		case PS_GLOBAL: return L.globals[o.index];
		case PS_OUT: return L.outp[o.index];
		default: return o.value;
	}
}
__device__ __forceinline__ void lane_write(const Lane& L, const ParticleOperand& o, float v) {
	switch (o.type) {
		case PS_CHANNEL: L.ch[(size_t)o.index * L.stride + L.slot] = v; break;
		case PS_REGISTER: L.regs[o.index * L.rstride + L.lane] = v; break;
		case PS_OUT: L.outp[o.index] = v; break;
		default: break;
	}
}

// SPLINE (run :785-796, processChunk :1207-1216): the quadratic through the midpoints of segment `u32(t)`, component `sub`. clamp(u32, 0, i32)
// is the unsigned minimum (core/math.h:520): a negative t of magnitude >= 1 converts to a large u32 and lands in the LAST segment.
__device__ __forceinline__ float p_spline(const ParticlesDevice& d, const ParticleSourceDev& s, float value, uint32_t sub) {
	const float t = f_mul(value, float(s.n_points - 2u));
	const uint32_t last = s.n_points - 3u;
	uint32_t seg = u32_x86(t);
	if (!(seg < last)) seg = last;
	const float rel = f_sub(t, float(seg));
	const float* q = d.spline_points + 3 * ((size_t)s.spline_at + seg) + sub;
	const float p1 = q[3];
	const float p0 = f_mul(f_add(p1, q[0]), 0.5f), p2 = f_mul(f_add(p1, q[6]), 0.5f);
	const float one_t = f_sub(1.f, rel);
	const float a = f_add(f_mul(p0, one_t), f_mul(p1, rel)), b = f_add(f_mul(p1, one_t), f_mul(p2, rel)); // lerp of core/math.cpp:190
	return f_add(f_mul(a, one_t), f_mul(b, rel));
}

// MESH's value (run :761-771): component `sub` of vertex `idx`, through Model::evalVertexPose where the model has bones. Only row `sub` of the
// blended matrix is formed, bone by bone in the reference's association ((a0 * w0 + a1 * w1) + a2 * w2) + a3 * w3.
__device__ __forceinline__ float p_mesh_vertex(const ParticlesDevice& d, const ParticleSourceDev& s, uint32_t idx, uint32_t sub) {
	const uint32_t vert = 3u * (s.mesh_at + idx); // (32-bit offsets from uniform bases: lmx_particles_add_mesh bounds the tables)
	if (!(s.flags & PARTICLE_SOURCE_BONES)) return d.mesh_positions[vert + sub];
	const char* skins = reinterpret_cast<const char*>(d.mesh_skins);
	const uint32_t skin = (s.skin_at + idx) * (uint32_t)sizeof(LmxSkin);
	const float4* pal = d.palette + 3 * (size_t)s.palette_at;
	float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	// One bone at a time, not unrolled: with the four bones' sixteen elements in flight at once the chunk kernels leave their 64 VGPRs
#pragma unroll 1
	for (uint32_t k = 0; k < 4; ++k) {
		uint32_t bone = *reinterpret_cast<const uint16_t*>(skins + (skin + (uint32_t)offsetof(LmxSkin, indices) + 2u * k));
		if (bone >= s.n_bones) bone = 0;
		const SkinRow e = skin_row(pal, bone, sub);
		const float w = *reinterpret_cast<const float*>(skins + (skin + 4u * k));
#pragma unroll
		for (int j = 0; j < 4; ++j) m[j] = k == 0 ? f_mul(e.e[j], w) : f_add(m[j], f_mul(e.e[j], w));
	}
	const float* p = d.mesh_positions;
	return f_add(f_add(f_add(f_mul(m[0], p[vert]), f_mul(m[1], p[vert + 1u])), f_mul(m[2], p[vert + 2u])), m[3]); // transformPoint, math.cpp:1231-1235
}

// ParticleSystem::run from record `ip` to the END that returns. True: the particle was killed.
__device__ __forceinline__ bool run_scalar(Lane L, const ParticleRec* prog, uint32_t ip) {
	bool killed = false;
	float* const outp = L.outp;
	for (;;) {
		const ParticleRec& r = prog[ip];
		uint32_t next = ip + 1;
		switch (r.op) {
			case P_END:
				if (r.kind == PE_RETURN) return killed;
				if (r.kind == PE_JUMP) next = r.a;
				if (r.kind == PE_EMIT_END) L.outp = outp;
				break;
			case P_EMIT: { // the block behind it writes its outputs into the particle's staging record of this EMIT (run :958-983)
				uint32_t* rec = L.stage + ((size_t)L.slot * L.n_emit + r.b) * PARTICLE_STAGE_WORDS;
				rec[0] = 1u;
				rec[1] = r.a;
				for (uint32_t k = 0; k < 16; ++k) rec[2 + k] = 0u;
				L.outp = reinterpret_cast<float*>(rec + 2);
				break;
			}
			case P_KILL: killed = true; break;
			case P_CMP: case P_CMP_ELSE:
				if (!(lane_read(L, r.o[0]) != 0.0f)) next = r.a;
				break;
			case P_RAND: lane_write(L, r.o[0], p_rand(L.seed, L.emitter, L.step, L.rslot, r.a, r.o[1].value, r.o[2].value)); break;
			case P_MESH: { // :741-774. Every `return` is the reference's: the run ends with its verdict so far
				const ParticleSourceDev s = L.dev->sources[L.system];
				if (!s.n_verts) return killed;
				float index = lane_read(L, r.o[1]);
				if (index < 0.0f) {
					index = float(p_draw(L.seed, L.emitter, L.step, L.rslot, MESH_DRAW_DOMAIN + r.a) % s.n_verts);
					lane_write(L, r.o[1], index);
				}
				if ((s.flags & PARTICLE_SOURCE_BONES) && s.palette_at == PARTICLE_NO_SOURCE) return killed;
				uint32_t idx = u32_x86(index + 0.5f);
				if (idx >= s.n_verts) idx = 0; // (the reference reads past the array)
				lane_write(L, r.o[0], p_mesh_vertex(*L.dev, s, idx, r.b));
				break;
			}
			case P_SPLINE: { // :775-798
				const ParticleSourceDev s = L.dev->sources[L.system];
				if (!s.n_points) return killed;
				lane_write(L, r.o[0], p_spline(*L.dev, s, lane_read(L, r.o[1]), r.b));
				break;
			}
			case P_MULTIPLY_ADD: lane_write(L, r.o[0], f_add(f_mul(lane_read(L, r.o[1]), lane_read(L, r.o[2])), lane_read(L, r.o[3]))); break;
			case P_MIX: { // lerp of core/math.cpp:190
				const float a = lane_read(L, r.o[1]), b = lane_read(L, r.o[2]), t = lane_read(L, r.o[3]);
				lane_write(L, r.o[0], f_add(f_mul(a, f_sub(1.f, t)), f_mul(b, t)));
				break;
			}
			case P_MOV: lane_write(L, r.o[0], lane_read(L, r.o[1])); break;
			case P_SIN: lane_write(L, r.o[0], f_sin(lane_read(L, r.o[1]))); break;
			case P_COS: lane_write(L, r.o[0], f_cos(lane_read(L, r.o[1]))); break;
			case P_SQRT: lane_write(L, r.o[0], f_sqrt(lane_read(L, r.o[1]))); break;
			case P_NOISE: lane_write(L, r.o[0], p_gnoise(lane_read(L, r.o[1]))); break;
			case P_NOT: lane_write(L, r.o[0], bits_f(lane_read(L, r.o[1]) == 0.0f ? 0xffffffffu : 0u)); break;
			default: {
				const float a = lane_read(L, r.o[1]), b = lane_read(L, r.o[2]);
				float v = 0.0f;
				switch (r.op) {
					case P_ADD: v = f_add(a, b); break;
					case P_SUB: v = f_sub(a, b); break;
					case P_MUL: v = f_mul(a, b); break;
					case P_DIV: v = f_div(a, b); break;
					case P_MOD: v = f_mod(a, b); break;
					case P_AND: v = (a != 0.0f && b != 0.0f) ? 1.f : 0.f; break;
					case P_OR: v = (a != 0.0f || b != 0.0f) ? 1.f : 0.f; break;
					case P_MAX: v = a > b ? a : b; break;
					case P_MIN: v = a < b ? a : b; break;
					case P_LT: v = a < b ? 1.f : 0.f; break;
					case P_GT: v = a > b ? 1.f : 0.f; break;
					default: break;
				}
				lane_write(L, r.o[0], v);
				break;
			}
		}
		ip = next;
	}
}

// One whole-chunk instruction for one lane (ProcessHelper::run1 / run2 / run3 and the cases of processChunk): the intrinsic form of core/simd.h
__device__ __forceinline__ void run_whole(const Lane& L, const ParticleRec& r, const ParticleGradient* gradients) {
	float v;
	switch (r.op) {
		case P_MOV: v = lane_read(L, r.o[1]); break;
		case P_SIN: v = f_sin(lane_read(L, r.o[1])); break;
		case P_COS: v = f_cos(lane_read(L, r.o[1])); break;
		case P_SQRT: v = f_sqrt(lane_read(L, r.o[1])); break;
		case P_NOISE: v = p_gnoise(lane_read(L, r.o[1])); break;
		case P_RAND: v = p_rand(L.seed, L.emitter, L.step, L.rslot, r.a, r.o[1].value, r.o[2].value); break;
		case P_SPLINE: v = p_spline(*L.dev, L.dev->sources[L.system], lane_read(L, r.o[1]), r.b); break; // (a system without a spline never gets here: the caller stops the program)
		case P_GRADIENT: {
			const ParticleGradient& g = gradients[r.a];
			const float arg = lane_read(L, r.o[1]);
			const float lo = g.keys[0], hi = g.keys[g.count - 1];
			const float m = arg > lo ? arg : lo;
			const float c = m < hi ? m : hi;
			uint32_t k = 1;
			while (k + 1 < g.count && c > g.keys[k]) ++k;
			v = f_sub(g.values[k], f_mul(f_sub(g.keys[k], c), g.ms[k]));
			break;
		}
		case P_MULTIPLY_ADD: v = f_add(f_mul(lane_read(L, r.o[1]), lane_read(L, r.o[2])), lane_read(L, r.o[3])); break;
		case P_MIX: {
			const float a = lane_read(L, r.o[1]), b = lane_read(L, r.o[2]), c = lane_read(L, r.o[3]);
			v = f_add(a, f_mul(f_sub(b, a), c));
			break;
		}
		case P_BLEND: { // _mm_blendv_ps(false_val, true_val, mask): the mask's sign bit selects
			const float fv = lane_read(L, r.o[1]), tv = lane_read(L, r.o[2]);
			v = (f_bits(lane_read(L, r.o[3])) & 0x80000000u) ? tv : fv;
			break;
		}
		default: {
			const float a = lane_read(L, r.o[1]), b = lane_read(L, r.o[2]);
			v = 0.0f;
			switch (r.op) {
				case P_ADD: v = f_add(a, b); break;
				case P_SUB: v = f_sub(a, b); break;
				case P_MUL: v = f_mul(a, b); break;
				case P_DIV: v = f_div(a, b); break;
				case P_MOD: v = f_mod(a, b); break;
				case P_AND: v = bits_f(f_bits(a) & f_bits(b)); break;
				case P_OR: v = bits_f(f_bits(a) | f_bits(b)); break;
				case P_MAX: v = a > b ? a : b; break; // _mm_max_ps: the second operand when either is NaN
				case P_MIN: v = a < b ? a : b; break;
				case P_LT: v = bits_f(a < b ? 0xffffffffu : 0u); break;
				case P_GT: v = bits_f(a > b ? 0xffffffffu : 0u); break;
				default: break;
			}
			break;
		}
	}
	lane_write(L, r.o[0], v);
}

__global__ void __launch_bounds__(PARTICLE_EMIT_BLOCK) k_particles_emit(ParticlesDevice d, const ParticleEmitJob* __restrict__ jobs, const ParticleRec* __restrict__ prog) {
	__shared__ float s_regs[PARTICLE_MAX_REGISTERS * PARTICLE_EMIT_BLOCK];
	const ParticleEmitJob job = jobs[blockIdx.y];
	const uint32_t i = blockIdx.x * PARTICLE_EMIT_BLOCK + threadIdx.x;
	if (i >= job.count) return;
	const ParticleEmitterDev em = d.emitters[job.emitter];
	const ParticleStateDev st = d.state[job.emitter];
	const uint32_t slot = st.count + i;
	if (slot < st.count || slot >= em.capacity) return; // past the reserved capacity: counted by k_particles_commit, not written
	for (uint32_t r = 0; r < PARTICLE_MAX_REGISTERS; ++r) s_regs[r * PARTICLE_EMIT_BLOCK + threadIdx.x] = 0.0f;
	Lane L;
	L.ch = d.channels + em.channel_base;
	L.stride = em.stride;
	L.slot = slot;
	L.rslot = slot; L.ribbon_index = 0.0f;
	L.regs = s_regs;
	L.rstride = PARTICLE_EMIT_BLOCK;
	L.lane = threadIdx.x;
	L.sysv = d.systems[em.system].values;
	L.globals = d.globals + d.systems[em.system].globals_at;
	L.outp = nullptr;
	float t = job.total_time; // the reference's repeated sum c1 + d + d + ..., not c1 + i * d
	if (job.time_step != 0.0f)
		for (uint32_t k = 0; k < i; ++k) t += job.time_step;
	L.total_time = t;
	L.emit_index = float(st.emit_index + i);
	L.emitting = true;
	L.seed = d.seed; L.emitter = job.emitter; L.step = d.step;
	L.stage = nullptr; L.n_emit = 0;
	L.dev = &d; L.system = em.system;
	(void)run_scalar(L, prog, em.prog_emit);
}

__global__ void k_particles_commit(ParticlesDevice d, const ParticleEmitJob* __restrict__ jobs, uint32_t n_jobs) {
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n_jobs) return;
	const ParticleEmitJob job = jobs[j];
	ParticleStateDev st = d.state[job.emitter];
	const uint32_t cap = d.emitters[job.emitter].capacity;
	const uint32_t room = cap - st.count;
	if (job.count > room) {
		st.count = cap;
		st.overflow = 1;
	} else {
		st.count += job.count;
	}
	st.emit_index += job.count;
	d.state[job.emitter] = st;
}

template <bool FILL> __global__ void __launch_bounds__(PARTICLE_BLOCK, 8) k_particles_chunk(ParticlesDevice d, const ParticleRec* __restrict__ prog, const ParticleGradient* __restrict__ gradients) {
	LMX_DYNAMIC_LDS(float, s_lds); // [registers][1024] register pages | [shadow channels][1024] | map[1024] | ballots[16 x 2] | kill count
	const uint32_t e = blockIdx.y;
	const ParticleStateDev st = d.state[e];
	const uint32_t from = blockIdx.x * PARTICLE_CHUNK;
	if (from >= st.count) return;
	const ParticleEmitterDev em = d.emitters[e];
	if (!FILL && d.level != 0xffffffffu && em.local != d.level) return;
	// (a ribbon emitter's points are k_particles_ribbon_chunk's: here its chunks have no particle, every lane idles through the program)
	const uint32_t n = em.ribbon_len ? 0u : min(PARTICLE_CHUNK, st.count - from), n4 = (n + 3u) & ~3u;
	const uint32_t lane = threadIdx.x;
	const bool active = lane < n4;
	const uint32_t n_shadow = FILL ? 0u : (uint32_t)__popc(em.shadow_mask);
	float* s_shadow = s_lds + em.registers * PARTICLE_CHUNK;
	uint32_t* s_map = reinterpret_cast<uint32_t*>(s_shadow + n_shadow * PARTICLE_CHUNK);
	uint32_t* s_ball = s_map + PARTICLE_CHUNK;
	uint32_t* s_kc = s_ball + 32;
	for (uint32_t r = 0; r < em.registers; ++r) s_lds[r * PARTICLE_CHUNK + lane] = 0.0f;
	if (!FILL && lane == 0) d.kill[em.kill_base + blockIdx.x] = 0;

	Lane L;
	L.ch = d.channels + em.channel_base;
	L.stride = em.stride;
	L.slot = from + lane;
	L.rslot = L.slot; L.ribbon_index = 0.0f;
	L.regs = s_lds;
	L.rstride = PARTICLE_CHUNK;
	L.lane = lane;
	L.sysv = d.systems[em.system].values;
	L.globals = d.globals + d.systems[em.system].globals_at;
	L.outp = FILL ? d.frame + d.slices[e].offset / 4 + (size_t)(from + lane) * em.outputs : nullptr;
	L.total_time = 0.0f;
	L.emit_index = L.sysv[PSV_EMIT_INDEX];
	L.emitting = false;
	L.seed = d.seed; L.emitter = e; L.step = d.step;
	L.stage = d.stage + em.stage_base;
	L.n_emit = FILL ? 0u : em.n_emit;
	L.dev = &d; L.system = em.system;
	if (active)
		for (uint32_t j = 0; j < L.n_emit; ++j) L.stage[((size_t)L.slot * L.n_emit + j) * PARTICLE_STAGE_WORDS] = 0u;

	uint32_t ip = FILL ? em.prog_output : em.prog_update;
	for (;;) {
		const ParticleRec& r = prog[ip];
		const uint32_t op = r.op;
		if (op == P_END) break;
		if (FILL && op == P_SPLINE && !d.sources[em.system].n_points) break; // processChunk :1196-1198 returns: uniform over the block, nothing behind it runs
		if (op != P_CMP && op != P_CMP_ELSE) {
			if (active) run_whole(L, r, gradients);
			++ip;
			continue;
		}
		// ---- a conditional block: per particle, then the kills in the reference's sequential order -----------------------------------
		const bool has_else = op == P_CMP_ELSE, kills = !FILL && (r.b & 1u) != 0;
		const uint32_t wmask = r.wmask;
		if (kills && active) { // the values a killed slot takes from a slot the loop has not visited yet are those from before the block
			uint32_t k = 0;
			for (uint32_t m = wmask; m; m &= m - 1, ++k) s_shadow[k * PARTICLE_CHUNK + lane] = L.ch[(size_t)(__ffs((int)m) - 1) * L.stride + L.slot];
		}
		bool killed = false;
		if (active) {
			const bool is_true = (f_bits(lane_read(L, r.o[0])) & 0x80000000u) && lane < n; // f4MoveMask: the sign bit
			if (is_true || has_else) killed = run_scalar(L, prog, is_true ? ip + 1 : r.a);
		}
		if (kills) {
			const unsigned long long ball = __ballot(killed);
			if ((lane & 63u) == 0) {
				s_ball[2 * (lane >> 6)] = (uint32_t)ball;
				s_ball[2 * (lane >> 6) + 1] = (uint32_t)(ball >> 32);
			}
			s_map[lane] = lane;
			__syncthreads();
			if (lane == 0) { // integer index logic only: `data[i] = data[last]; --last` for every kill, ascending
				int32_t last = (int32_t)n - 1;
				uint32_t kc = 0;
				for (uint32_t w = 0; w < 32; ++w) {
					for (uint32_t bits = s_ball[w]; bits; bits &= bits - 1) {
						const int32_t i = (int32_t)(w * 32u) + __ffs((int)bits) - 1;
						++kc;
						if (last >= 0) { // (below the chunk the reference reads its neighbour: unspecified, nothing moves here)
							if (last > i) s_map[i] = (uint32_t)last | MAP_PRE;
							else if (last < i) s_map[i] = s_map[last];
						}
						--last;
					}
				}
				*s_kc = kc;
				if (kc) d.kill[em.kill_base + blockIdx.x] = kc;
			}
			__syncthreads();
			if (*s_kc) {
				const uint32_t mp = s_map[lane], src = mp & 0x3ffu;
				const bool moved = active && mp != lane;
				for (uint32_t c = 0; c < em.channels; ++c) {
					float v = 0.0f;
					if (moved) {
						if ((mp & MAP_PRE) && ((wmask >> c) & 1u)) v = s_shadow[(uint32_t)__popc(wmask & ((1u << c) - 1u)) * PARTICLE_CHUNK + src];
						else v = L.ch[(size_t)c * L.stride + from + src];
					}
					__syncthreads();
					if (moved) L.ch[(size_t)c * L.stride + L.slot] = v;
				}
			}
			__syncthreads(); // s_map / s_kc are rewritten by the next block
		}
		ip = r.c;
	}
}

__global__ void k_particles_plan(ParticlesDevice d) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= d.n_emitters) return;
	ParticleStateDev st = d.state[e];
	const ParticleEmitterDev& em = d.emitters[e]; // (read in place: emit_group is indexed by a loop counter)
	if (d.level != 0xffffffffu && em.local != d.level) return;
	if (em.ribbon_len) return; // no kills, no EMIT: nothing to plan
	uint32_t n_ops = 0, n_sub = 0;
	const uint32_t updated = st.count; // what the chunk kernel ran over
	st.killed = 0;
	if (st.count) {
		uint32_t* kc = d.kill + em.kill_base;
		ParticleCopyOp* ops = d.ops + em.kill_base;
		const uint32_t chunks = (st.count + PARTICLE_CHUNK - 1) / PARTICLE_CHUNK;
		uint32_t head = 0, tail = chunks - 1, total = 0;
		for (uint32_t i = 0; i < chunks; ++i) total += kc[i];
		while (head != tail) {
			const uint32_t kh = kc[head];
			if (kh == 0) {
				++head;
				continue;
			}
			const uint32_t tail_start = PARTICLE_CHUNK * tail;
			const uint32_t tail_count = min(PARTICLE_CHUNK, st.count - tail_start) - kc[tail];
			ParticleCopyOp op;
			op.dst = head * PARTICLE_CHUNK + PARTICLE_CHUNK - kh;
			op.pad = 0;
			if (tail_count <= kh) {
				op.src = tail_start;
				op.len = tail_count;
				--tail;
				kc[head] = kh - tail_count;
			} else {
				op.src = tail_start + tail_count - kh;
				op.len = kh;
				kc[tail] += kh;
				++head;
			}
			// (kill counts beyond a chunk's particles are outside what the reference defines: such a copy is dropped, never out of bounds)
			if (op.len && op.len <= PARTICLE_CHUNK && op.dst <= em.capacity - op.len && op.src <= em.capacity - op.len && n_ops < em.max_chunks) ops[n_ops++] = op;
			if (tail_count > PARTICLE_CHUNK) break;
		}
		st.killed = total;
		st.count = total < st.count ? st.count - total : 0;
	}
	// The drain of :1558-1571, integer part: the staged EMIT records in the reference's order - chunk by chunk, within a chunk conditional
	// block by block, particle by particle - each takes init_emit_count slots of its target (past the capacity: counted, not written).
	if (em.n_emit && updated) {
		const uint32_t* stage = d.stage + em.stage_base;
		ParticleSubJob* jobs = d.sub_jobs + em.job_base;
		for (uint32_t from = 0; from < updated; from += PARTICLE_CHUNK) {
			const uint32_t to4 = from + ((min(PARTICLE_CHUNK, updated - from) + 3u) & ~3u);
			for (uint32_t j0 = 0; j0 < em.n_emit;) {
				uint32_t j1 = j0 + 1;
				while (j1 < em.n_emit && em.emit_group[j1] == em.emit_group[j0]) ++j1;
				for (uint32_t p = from; p < to4; ++p)
					for (uint32_t j = j0; j < j1; ++j) {
						const uint32_t at = p * em.n_emit + j;
						const uint32_t* rec = stage + (size_t)at * PARTICLE_STAGE_WORDS;
						if (!rec[0]) continue;
						const uint32_t t = em.first_of_system + rec[1];
						ParticleStateDev ts = t == e ? st : d.state[t];
						const uint32_t want = d.emitters[t].init_emit_count, room = d.emitters[t].capacity - ts.count;
						ParticleSubJob job;
						job.stage_index = at; job.target = t; job.slot = ts.count; job.emit_index = ts.emit_index; job.n = min(want, room);
						if (want > room) ts.overflow = 1;
						ts.count += job.n;
						ts.emit_index += want;
						if (t == e) st = ts;
						else d.state[t] = ts;
						jobs[n_sub++] = job;
					}
				j0 = j1;
			}
		}
	}
	d.n_ops[e] = n_ops;
	d.n_sub[e] = n_sub;
	d.state[e] = st;
}

// ParticleSystem::emit of every drained record: the target's emit program once per new particle, the record's outputs in its first registers,
// time_step = 0
__global__ void __launch_bounds__(PARTICLE_EMIT_BLOCK) k_particles_subemit(ParticlesDevice d, const ParticleRec* __restrict__ prog) {
	__shared__ float s_regs[PARTICLE_MAX_REGISTERS * PARTICLE_EMIT_BLOCK];
	const uint32_t e = blockIdx.y;
	const ParticleEmitterDev src = d.emitters[e];
	if (!src.n_emit || (d.level != 0xffffffffu && src.local != d.level)) return;
	const uint32_t n_sub = d.n_sub[e];
	for (uint32_t r = blockIdx.x; r < n_sub; r += gridDim.x) {
		const ParticleSubJob job = d.sub_jobs[src.job_base + r];
		const ParticleEmitterDev em = d.emitters[job.target];
		const float* in = reinterpret_cast<const float*>(d.stage + src.stage_base + (size_t)job.stage_index * PARTICLE_STAGE_WORDS + 2);
		for (uint32_t i = threadIdx.x; i < job.n; i += PARTICLE_EMIT_BLOCK) {
			for (uint32_t k = 0; k < PARTICLE_MAX_REGISTERS; ++k) s_regs[k * PARTICLE_EMIT_BLOCK + threadIdx.x] = k < em.emit_inputs ? in[k] : 0.0f;
			Lane L;
			L.ch = d.channels + em.channel_base;
			L.stride = em.stride;
			L.slot = job.slot + i;
			L.rslot = L.slot; L.ribbon_index = 0.0f;
			L.regs = s_regs;
			L.rstride = PARTICLE_EMIT_BLOCK;
			L.lane = threadIdx.x;
			L.sysv = d.systems[em.system].values;
			L.globals = d.globals + d.systems[em.system].globals_at;
			L.outp = nullptr;
			L.total_time = L.sysv[PSV_TOTAL_TIME];
			L.emit_index = float(job.emit_index + i);
			L.emitting = true;
			L.seed = d.seed; L.emitter = job.target; L.step = d.step;
			L.stage = nullptr; L.n_emit = 0;
			L.dev = &d; L.system = em.system;
			(void)run_scalar(L, prog, em.prog_emit);
		}
	}
}

__global__ void __launch_bounds__(PARTICLE_BLOCK) k_particles_compact(ParticlesDevice d) {
	const uint32_t e = blockIdx.y;
	const ParticleEmitterDev em = d.emitters[e];
	if (d.level != 0xffffffffu && em.local != d.level) return;
	if (blockIdx.x >= d.n_ops[e]) return;
	const ParticleCopyOp op = d.ops[em.kill_base + blockIdx.x];
	if (threadIdx.x >= op.len) return;
	float* ch = d.channels + em.channel_base;
	for (uint32_t c = 0; c < em.channels; ++c) ch[(size_t)c * em.stride + op.dst + threadIdx.x] = ch[(size_t)c * em.stride + op.src + threadIdx.x];
}

__global__ void __launch_bounds__(PARTICLE_SCAN_BLOCK) k_particles_slices(ParticlesDevice d) {
	__shared__ uint32_t s_sum[PARTICLE_SCAN_BLOCK];
	const uint32_t t = threadIdx.x;
	const uint32_t per = (d.n_emitters + PARTICLE_SCAN_BLOCK - 1) / PARTICLE_SCAN_BLOCK;
	const uint32_t first = min(t * per, d.n_emitters), end = min(first + per, d.n_emitters);
	uint32_t mine = 0;
	for (uint32_t e = first; e < end; ++e) mine += ((d.state[e].count + 3u) & ~3u) * d.emitters[e].outputs * 4u;
	s_sum[t] = mine;
	__syncthreads();
	for (uint32_t step = 1; step < PARTICLE_SCAN_BLOCK; step <<= 1) {
		const uint32_t add = t >= step ? s_sum[t - step] : 0u;
		__syncthreads();
		s_sum[t] += add;
		__syncthreads();
	}
	uint32_t offset = s_sum[t] - mine;
	for (uint32_t e = first; e < end; ++e) {
		const uint32_t count = d.state[e].count, bytes = ((count + 3u) & ~3u) * d.emitters[e].outputs * 4u;
		LmxParticleSlice s;
		s.offset = offset; // a multiple of 16: every slice is a whole number of four-particle rows of floats
		s.bytes = bytes;
		s.particles = count;
		s.outputs_count = d.emitters[e].outputs;
		d.slices[e] = s;
		offset += bytes;
	}
}

// ---- ribbon emitters ----------------------------------------------------------------------------------------------------
// A ribbon's {offset, length, emit_index} is host state (every count that moves it is known there); the device gets it in the jobs and in
// the ParticleRibbonDev table and needs neither counters nor atomics.

// ParticleSystem::emitRibbonPoints (:358-409) of every job of a pass. Point i of a call lands in ring slot (offset0 + length0 + i) % ribbon_len,
// so lane j of a job owns the slot of points j, j + ribbon_len, ... and runs them in order: no two lanes write one slot. (The reference
// takes the modulus of a u32 sum; the two agree until offset + length passes 2^32, which is where the slots are computed as it does.)
__global__ void __launch_bounds__(PARTICLE_EMIT_BLOCK, 6) k_particles_ribbon_emit(ParticlesDevice d, const ParticleRibbonJob* __restrict__ jobs, uint32_t n_jobs, uint32_t total_lanes, const ParticleRec* __restrict__ prog) {
	__shared__ float s_regs[PARTICLE_MAX_REGISTERS * PARTICLE_EMIT_BLOCK];
	const uint32_t g = blockIdx.x * PARTICLE_EMIT_BLOCK + threadIdx.x;
	if (g >= total_lanes) return;
	uint32_t lo = 0, hi = n_jobs; // the last job whose first lane is <= g
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (jobs[mid].first_lane <= g) lo = mid;
		else hi = mid;
	}
	const ParticleRibbonJob job = jobs[lo];
	const ParticleEmitterDev em = d.emitters[job.emitter];
	const uint32_t len = em.ribbon_len;
	if (!len || job.ring >= em.max_ribbons || job.length0 > len) return;
	const uint32_t room = len - job.length0; // points that still grow the ribbon; the rest advance its offset
	Lane L;
	L.ch = d.channels + em.channel_base + (size_t)job.ring * len;
	L.stride = em.stride;
	L.ribbon_index = float(job.ribbon);
	L.regs = s_regs;
	L.rstride = PARTICLE_EMIT_BLOCK;
	L.lane = threadIdx.x;
	L.sysv = d.systems[em.system].values;
	L.globals = d.globals + d.systems[em.system].globals_at;
	L.outp = nullptr;
	L.emitting = true;
	L.seed = d.seed; L.emitter = job.emitter; L.step = d.step;
	L.stage = nullptr; L.n_emit = 0;
	L.dev = &d; L.system = em.system;
	float t = job.total_time; // the repeated sum c1 + d + d + ..., restarted for every ribbon
	uint64_t summed = 0;
	for (uint64_t i = g - job.first_lane; i < job.count; i += len) {
		if (job.time_step != 0.0f)
			for (; summed < i; ++summed) t += job.time_step;
		const uint32_t length = i < room ? job.length0 + (uint32_t)i + 1u : len;
		const uint32_t offset = i < room ? job.offset0 : job.offset0 + ((uint32_t)i + 1u - room);
		L.slot = (offset + length - 1u) % len;
		L.rslot = job.ribbon * len + L.slot;
		for (uint32_t r = 0; r < PARTICLE_MAX_REGISTERS; ++r) s_regs[r * PARTICLE_EMIT_BLOCK + threadIdx.x] = 0.0f;
		L.total_time = t;
		L.emit_index = float(job.emit_index0 + (uint32_t)i);
		(void)run_scalar(L, prog, em.prog_emit);
	}
}

__global__ void k_particles_ribbon_commit(ParticlesDevice d) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= d.n_ribbon_emitters) return;
	const ParticleRibbonCount rc = d.ribbon_counts[k];
	d.state[rc.emitter].count = rc.total;
}

// processChunk over the ribbons of every ribbon emitter: a block takes floor(1024 / ribbon_len) whole ribbons, lane -> (ribbon, ring slot)
// is fixed per emitter. <false>: the update program over ring slots [0, (length + 3) & ~3) as updateRibbons' chunk covers them (:1431-1439;
// it does not follow `offset`). <true>: the output program over [0, length), each slot into its row of the ribbon's packed rows. Ribbon
// emitters hold no KILL and no EMIT (refused when the program is set), so a conditional block is the per-lane interpreter and nothing more.
template <bool FILL> __global__ void __launch_bounds__(PARTICLE_BLOCK) k_particles_ribbon_chunk(ParticlesDevice d, const ParticleRec* __restrict__ prog, const ParticleGradient* __restrict__ gradients) {
	LMX_DYNAMIC_LDS(float, s_lds); // [registers][1024] register pages
	const ParticleRibbonCount rc = d.ribbon_counts[blockIdx.y];
	const ParticleEmitterDev em = d.emitters[rc.emitter];
	const uint32_t len = em.ribbon_len;
	if (!len) return;
	const uint32_t per = PARTICLE_CHUNK / len, first = blockIdx.x * per;
	if (first >= rc.n_ribbons) return;
	const uint32_t lane = threadIdx.x;
	const uint32_t rl = lane / len, slot = lane - rl * len, ribbon = first + rl;
	const bool live = rl < per && ribbon < rc.n_ribbons && ribbon < em.max_ribbons;
	ParticleRibbonDev rb;
	rb.ring = rb.length = rb.row = rb.pad = 0;
	if (live) rb = d.ribbons[em.ribbon_base + ribbon];
	const uint32_t n = min(rb.length, len);
	const bool active = live && rb.ring < em.max_ribbons && slot < (FILL ? n : (n + 3u) & ~3u);
	for (uint32_t r = 0; r < em.registers; ++r) s_lds[r * PARTICLE_CHUNK + lane] = 0.0f;

	Lane L;
	L.ch = d.channels + em.channel_base + (size_t)rb.ring * len;
	L.stride = em.stride;
	L.slot = slot;
	L.rslot = ribbon * len + slot;
	L.ribbon_index = float(ribbon);
	L.regs = s_lds;
	L.rstride = PARTICLE_CHUNK;
	L.lane = lane;
	L.sysv = d.systems[em.system].values;
	L.globals = d.globals + d.systems[em.system].globals_at;
	L.outp = FILL ? d.frame + d.slices[rc.emitter].offset / 4 + (size_t)(rb.row + slot) * em.outputs : nullptr;
	L.total_time = 0.0f;
	L.emit_index = L.sysv[PSV_EMIT_INDEX];
	L.emitting = false;
	L.seed = d.seed; L.emitter = rc.emitter; L.step = d.step;
	L.dev = &d; L.system = em.system;
	L.stage = d.stage; L.n_emit = 0; // never used: no program of a ribbon emitter holds an EMIT (a null pointer here crashes ROCm 7.2's clang in SimplifyCFG)

	uint32_t ip = FILL ? em.prog_output : em.prog_update;
	for (;;) {
		const ParticleRec& r = prog[ip];
		const uint32_t op = r.op;
		if (op == P_END) break;
		if (FILL && op == P_SPLINE && !d.sources[em.system].n_points) break; // processChunk :1196-1198 returns: uniform over the block, nothing behind it runs
		if (op != P_CMP && op != P_CMP_ELSE) {
			if (active) run_whole(L, r, gradients);
			++ip;
			continue;
		}
		if (active) {
			const bool is_true = (f_bits(lane_read(L, r.o[0])) & 0x80000000u) && slot < n;
			if (is_true || op == P_CMP_ELSE) (void)run_scalar(L, prog, is_true ? ip + 1 : r.a);
		}
		ip = r.c;
	}
}

} // namespace

size_t particle_chunk_lds_bytes(uint32_t registers, uint32_t shadow_channels) {
	return ((size_t)registers + shadow_channels + 1) * PARTICLE_CHUNK * sizeof(float) + 33 * sizeof(uint32_t);
}

hipError_t launch_particles_emit(hipStream_t s, const ParticlesDevice& d, const ParticleEmitJob* jobs, uint32_t n_jobs, uint32_t max_count) {
	if (!n_jobs) return hipSuccess;
	if (max_count) {
		hipLaunchKernelGGL(k_particles_emit, dim3((max_count + PARTICLE_EMIT_BLOCK - 1) / PARTICLE_EMIT_BLOCK, n_jobs), dim3(PARTICLE_EMIT_BLOCK), 0, s, d, jobs, d.prog);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_particles_commit, dim3((n_jobs + 255) / 256), dim3(256), 0, s, d, jobs, n_jobs);
	return hipGetLastError();
}

template <bool FILL> static hipError_t launch_chunks(hipStream_t s, const ParticlesDevice& d, uint32_t max_chunks, size_t lds) {
#ifndef LMX_HOSTSIM
	if (lds > 64 * 1024) { // beyond the default limit of a launch's dynamic LDS (the CU holds 160 KiB)
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_particles_chunk<FILL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
#endif
	hipLaunchKernelGGL(k_particles_chunk<FILL>, dim3(max_chunks, d.n_emitters), dim3(PARTICLE_BLOCK), lds, s, d, d.prog, d.gradients);
	return hipGetLastError();
}

hipError_t launch_particles_update(hipStream_t s, const ParticlesDevice& d, uint32_t max_chunks, uint32_t max_registers, uint32_t max_shadow, bool sub_emit) {
	if (!d.n_emitters || !max_chunks) return hipSuccess;
	hipError_t e = launch_chunks<false>(s, d, max_chunks, particle_chunk_lds_bytes(max_registers, max_shadow));
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_particles_plan, dim3((d.n_emitters + 63) / 64), dim3(64), 0, s, d);
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_particles_compact, dim3(max_chunks, d.n_emitters), dim3(PARTICLE_BLOCK), 0, s, d);
	e = hipGetLastError();
	if (e != hipSuccess || !sub_emit) return e;
	hipLaunchKernelGGL(k_particles_subemit, dim3(PARTICLE_SUB_BLOCKS, d.n_emitters), dim3(PARTICLE_EMIT_BLOCK), 0, s, d, d.prog);
	return hipGetLastError();
}

hipError_t launch_particles_fill(hipStream_t s, const ParticlesDevice& d, uint32_t max_chunks, uint32_t max_registers) {
	if (!d.n_emitters) return hipSuccess;
	hipLaunchKernelGGL(k_particles_slices, dim3(1), dim3(PARTICLE_SCAN_BLOCK), 0, s, d);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess || !max_chunks) return e;
	return launch_chunks<true>(s, d, max_chunks, particle_chunk_lds_bytes(max_registers, 0));
}

hipError_t launch_particles_ribbon_emit(hipStream_t s, const ParticlesDevice& d, const ParticleRibbonJob* jobs, uint32_t n_jobs, uint32_t total_lanes) {
	if (!n_jobs || !total_lanes) return hipSuccess;
	hipLaunchKernelGGL(k_particles_ribbon_emit, dim3((total_lanes + PARTICLE_EMIT_BLOCK - 1) / PARTICLE_EMIT_BLOCK), dim3(PARTICLE_EMIT_BLOCK), 0, s, d, jobs, n_jobs, total_lanes, d.prog);
	return hipGetLastError();
}

hipError_t launch_particles_ribbon_commit(hipStream_t s, const ParticlesDevice& d) {
	if (!d.n_ribbon_emitters) return hipSuccess;
	hipLaunchKernelGGL(k_particles_ribbon_commit, dim3((d.n_ribbon_emitters + 255) / 256), dim3(256), 0, s, d);
	return hipGetLastError();
}

template <bool FILL> static hipError_t launch_ribbon_chunks(hipStream_t s, const ParticlesDevice& d, uint32_t max_groups, uint32_t max_registers) {
	if (!d.n_ribbon_emitters || !max_groups) return hipSuccess;
	const size_t lds = (size_t)max_registers * PARTICLE_CHUNK * sizeof(float);
#ifndef LMX_HOSTSIM
	if (lds > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_particles_ribbon_chunk<FILL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
#endif
	hipLaunchKernelGGL(k_particles_ribbon_chunk<FILL>, dim3(max_groups, d.n_ribbon_emitters), dim3(PARTICLE_BLOCK), lds, s, d, d.prog, d.gradients);
	return hipGetLastError();
}

hipError_t launch_particles_ribbon_update(hipStream_t s, const ParticlesDevice& d, uint32_t max_groups, uint32_t max_registers) { return launch_ribbon_chunks<false>(s, d, max_groups, max_registers); }
hipError_t launch_particles_ribbon_fill(hipStream_t s, const ParticlesDevice& d, uint32_t max_groups, uint32_t max_registers) { return launch_ribbon_chunks<true>(s, d, max_groups, max_registers); }

} // namespace lmx
