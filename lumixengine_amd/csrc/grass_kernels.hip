// grass_kernels.hip — Terrain::createGrass's quads (renderer/terrain.cpp:86-135) and the quad loop of PipelineImpl::renderGrass
// (renderer/pipeline.cpp:2160-2199). FMA-free (-ffp-contract=off), fp32 with IEEE divisions and roots; the random floats are fp64 products
// rounded to fp32 as RandomGenerator::randFloat rounds them (core/math.cpp:1372-1378).
//
//   k_grass_quads  ONE WAVE per new quad.
//                  A  the lanes stage the quad's window of the splatmap into LDS: of `splat >> 16` the one byte that holds the quad's
//                     type bit; texels outside the map are 0. A window wider than GRASS_WINDOW per side is not staged: the chain reads global.
//                  B  lane 0 runs the reference's chain: 1024 iterations of the two generators, the two products, the division and the
//                     lookup. How many draws an iteration consumes depends on whether its own sample was accepted, so the iterations are
//                     one sequence. An accepted sample leaves {pn.x, pn.y, u, v} - the generators behind the position draws - on an LDS
//                     list and the chain steps over its scale and rotation draws.
//                  C  lane l takes the accepted samples l, l + 64, ...: the remaining draws from the stored state, the interpolated
//                     height (lmx_terrain_height.h, shared with the ray cast), the scale and the rotation, and writes the record to
//                     slots 2 t and 2 t + 1 of the quad's slice (`instances.emplace()` then `instances.push(inst)`, :102 / :121) with
//                     16-byte stores. A wave reduction gives the AABB, lane 0 writes the quad record.
//                  Argument order: `Vec2(rg.randFloat(), rg.randFloat())` and the Vec3 of ALL_RANDOM are evaluated right to left, as g++
//                  evaluates them: the first draw is pn.y, then pn.x; axis.z, axis.y, axis.x.
//   k_grass_cull   ONE BLOCK per view walks the live-quad list in tiles of GRASS_CULL_BLOCK, one lane per (view, quad): the six planes of
//                  frustum.getRelative(tr.pos).intersectAABB, the distance, count_scale and the truncation. Survivors are compacted in list
//                  order by ballot, a per-wave count in LDS and the block's running base: no atomics, so two runs give the same bytes.
#include "lmx_grass.h"
#include "lmx_terrain_height.h"

#include <float.h>

namespace lmx {

namespace {

constexpr uint32_t WAVE = 64;
constexpr float GRASS_PI = 3.14159265f; // core/math.h: PI

// the library's sine and cosine are long expansions with fused multiply-adds of their own: tests/test_isa_grass_kernels.py compiles the
// file a second time without them, and what is left must hold none
#ifdef LMX_GRASS_NO_LIBM
__device__ __forceinline__ float sin_of(float a) { return a * 0.5f; }
__device__ __forceinline__ float cos_of(float a) { return a * 0.25f; }
#else
__device__ __forceinline__ float sin_of(float a) { return sinf(a); }
__device__ __forceinline__ float cos_of(float a) { return cosf(a); }
#endif

// u32(v) as g++ compiles it for x86-64: cvttss2si into a 64-bit register, of which the low half is kept. NaN and |v| >= 2^63 give 0.
__device__ __forceinline__ uint32_t u32_of(float v) {
	if (v >= 0.0f && v < 4294967296.0f) return (uint32_t)v;
	if (v >= -9223372036854775808.0f && v < 9223372036854775808.0f) return (uint32_t)(unsigned long long)(long long)v;
	return 0u;
}

struct Rng { // RandomGenerator, core/math.cpp:1333-1341: two 16-bit multiply-with-carry generators
	uint32_t u, v;
	__device__ __forceinline__ uint32_t rand() {
		u = 36969u * (u & 65535u) + (u >> 16);
		v = 18000u * (v & 65535u) + (v >> 16);
		return (u << 16) + v;
	}
	__device__ __forceinline__ float rand_float() { return (float)((double)rand() * 2.328306435996595e-10); }                  // :1376-1378
	__device__ __forceinline__ float rand_float(float from, float to) { return from + (float)((double)(to - from) * ((double)rand() * 2.328306435996595e-10)); } // :1372-1374
};

// the byte of `getPixelNearest(x, z) >> 16` that holds the type's bit (texture.cpp:90-95: 0 outside the map)
__device__ __forceinline__ uint32_t splat_byte(const GrassTerrainDev& te, const uint8_t* texels, uint32_t x, uint32_t z, uint32_t shift) {
	if (!te.splat_ok || x >= te.splat_w || z >= te.splat_h) return 0u;
	const uint32_t texel = reinterpret_cast<const uint32_t*>(texels + te.splat_at)[(size_t)z * te.splat_w + x]; // (< w * h <= 2^30: checked when the table was set)
	return (texel >> shift) & 0xffu;
}

// AABB::addPoint's fold (geometry.cpp:535-538, minimum / maximum of core/math.h): a point replaces the bound only when it is strictly
// beyond it, so among equal values (+0 and -0) the EARLIEST sample stays. `at` = the sample's place in the sequence.
struct Bound { float v; uint32_t at; };
__device__ __forceinline__ Bound lower_of(Bound a, Bound b) { return (b.v < a.v || (b.v == a.v && b.at < a.at)) ? b : a; }
__device__ __forceinline__ Bound upper_of(Bound a, Bound b) { return (b.v > a.v || (b.v == a.v && b.at < a.at)) ? b : a; }
__device__ __forceinline__ Bound wave_fold(Bound b, bool lower) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		Bound o;
		o.v = __shfl_xor(b.v, m);
		o.at = __shfl_xor(b.at, m);
		b = lower ? lower_of(b, o) : upper_of(b, o);
	}
	return b;
}

__global__ __launch_bounds__(GRASS_BLOCK) void k_grass_quads(GrassQuadsDevice d) {
	__shared__ uint8_t s_window[GRASS_WINDOW * GRASS_WINDOW];
	__shared__ float4 s_list[LMX_GRASS_SAMPLES]; // {pn.x, pn.y, u, v}
	__shared__ uint32_t s_accepted;
	const uint32_t lane = threadIdx.x;
	const GrassJob job = d.jobs[blockIdx.x];
	const GrassTerrainDev te = d.terrains[job.terrain];
	const float quad_size = job.spacing * 32;                      // Vec2 quad_size(type.m_spacing * 32), :61
	const float from_x = (float)job.i * quad_size, from_z = (float)job.j * quad_size; // Vec2((float)i, (float)j) * quad_size, :87
	const float sx = te.scale[0];
	const uint32_t shift = 16u + (job.type & 8u), bit = 1u << (job.type & 7u); // (splat >> 16) & (1 << type_idx), :99

	// A. every sample's p lies in [from, from + quad_size] (pn <= 1, each operation rounds monotonically), so its texel lies in this window
	const uint32_t x0 = u32_of(from_x / sx), x1 = u32_of((from_x + quad_size) / sx);
	const uint32_t z0 = u32_of(from_z / sx), z1 = u32_of((from_z + quad_size) / sx);
	const bool staged = te.splat_ok && x1 >= x0 && z1 >= z0 && x1 - x0 < GRASS_WINDOW && z1 - z0 < GRASS_WINDOW;
	const uint32_t ww = staged ? x1 - x0 + 1 : 0u, wh = staged ? z1 - z0 + 1 : 0u;
	for (uint32_t t = lane; t < ww * wh; t += GRASS_BLOCK) s_window[t] = (uint8_t)splat_byte(te, d.texels, x0 + t % ww, z0 + t / ww, shift);
	__syncthreads();

	// B. the chain
	if (lane == 0) {
		uint32_t n = 0;
		if (te.splat_ok) { // (a map that gives 0 everywhere accepts nothing: no sample's draws matter)
			Rng rg = {job.i + 13u, job.j + 57u}; // :91
			const uint32_t skip = job.rotation_mode == LMX_GRASS_ROTATION_ALL_RANDOM ? 5u : 2u; // the scale, then 4 or 1 rotation draws
			for (uint32_t k = 0; k < LMX_GRASS_SAMPLES; ++k) {
				const float pn_y = rg.rand_float(); // Vec2(rg.randFloat(), rg.randFloat()): right to left
				const float pn_x = rg.rand_float();
				const float px = from_x + pn_x * quad_size; // :96-97
				const float pz = from_z + pn_y * quad_size;
				const uint32_t tx = u32_of(px / sx), tz = u32_of(pz / sx); // :98
				const uint32_t wx = tx - x0, wz = tz - z0;
				const uint32_t byte = (wx < ww && wz < wh) ? s_window[wz * ww + wx] : splat_byte(te, d.texels, tx, tz, shift);
				if (byte & bit) {
					s_list[n++] = make_float4(pn_x, pn_y, __uint_as_float(rg.u), __uint_as_float(rg.v));
					for (uint32_t s = 0; s < skip; ++s) rg.rand();
				}
			}
		}
		s_accepted = n;
	}
	__syncthreads();

	// C. the records
	const uint32_t n_acc = s_accepted;
	TerrainView tv;
	tv.texels = d.texels + te.height_at; tv.w = (int32_t)te.width; tv.h = (int32_t)te.height; tv.format = te.format;
	tv.sx = te.scale[0]; tv.sy = te.scale[1]; tv.sz = te.scale[2];
	float4* slice = d.pool + (size_t)job.slot * (2 * LMX_GRASS_SLOT_INSTANCES);
	Bound lo[3], hi[3];
	for (int c = 0; c < 3; ++c) { // AABB aabb(Vec3(FLT_MAX), Vec3(-FLT_MAX)), :90: ahead of every sample
		lo[c] = Bound{FLT_MAX, 0u};
		hi[c] = Bound{-FLT_MAX, 0u};
	}
	for (uint32_t t = lane; t < n_acc; t += GRASS_BLOCK) {
		const float4 e = s_list[t];
		Rng rg = {__float_as_uint(e.z), __float_as_uint(e.w)};
		const float px = from_x + e.x * quad_size;
		const float pz = from_z + e.y * quad_size;
		const float py = terrain_height(tv, px, pz);     // :100
		const float scale = rg.rand_float(0.7f, 1.0f);   // :101
		float4 rot;
		if (job.rotation_mode == LMX_GRASS_ROTATION_ALL_RANDOM) { // :111-114
			const float rz = rg.rand_float(), ry = rg.rand_float(), rx = rg.rand_float(); // Vec3(r, r, r): right to left
			const V3 axis = normalize(V3{rx * 2.0f - 1.0f, ry * 2.0f - 1.0f, rz * 2.0f - 1.0f});
			const float half_angle = (rg.rand_float() * 2 * GRASS_PI) * 0.5f; // Quat(axis, angle), math.cpp:570-578
			const float s = sin_of(half_angle);
			rot = make_float4(axis.x * s, axis.y * s, axis.z * s, cos_of(half_angle));
		} else { // Y_UP, :106-109
			const float angle = rg.rand_float();
			rot = make_float4(0.0f, sin_of(angle * GRASS_PI), 0.0f, cos_of(angle * GRASS_PI));
		}
		const float4 ps = make_float4(px, py, pz, scale);
		float4* r = slice + 4 * (size_t)t; // records 2 t and 2 t + 1
		r[0] = ps; r[1] = rot; r[2] = ps; r[3] = rot;
		const float p[3] = {px, py, pz};
		for (int c = 0; c < 3; ++c) {
			lo[c] = lower_of(lo[c], Bound{p[c], t + 1});
			hi[c] = upper_of(hi[c], Bound{p[c], t + 1});
		}
	}
	for (int c = 0; c < 3; ++c) {
		lo[c] = wave_fold(lo[c], true);
		hi[c] = wave_fold(hi[c], false);
	}
	if (lane == 0) {
		LmxGrassQuad q;
		for (int c = 0; c < 3; ++c) { q.aabb_min[c] = lo[c].v; q.aabb_max[c] = hi[c].v; }
		q.ij[0] = (int32_t)job.i; q.ij[1] = (int32_t)job.j; // IVec2(i, j), :128
		q.type = job.type;
		q.instances_count = 2 * n_acc;
		q.terrain = job.terrain;
		q.slot = job.slot;
		d.quads[job.slot] = q;
	}
}

__global__ __launch_bounds__(GRASS_CULL_BLOCK) void k_grass_cull(GrassCullDevice d) {
	constexpr uint32_t WAVES = GRASS_CULL_BLOCK / WAVE;
	__shared__ uint32_t s_wave[WAVES];
	__shared__ uint32_t s_sum[2][WAVES];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, view = blockIdx.x;
	const GrassViewDev& v = d.views[view];
	LmxGrassDraw* out = d.draws + (size_t)view * d.draw_stride;
	uint32_t base = 0, culled = 0, instances = 0; // base: block-uniform
	for (uint32_t q0 = 0; q0 < d.n_live; q0 += GRASS_CULL_BLOCK) {
		const uint32_t qi = q0 + tid;
		bool draw = false;
		LmxGrassDraw rec;
		rec.quad = qi; rec.slot = 0; rec.terrain = 0; rec.type = 0; rec.instance_count = 0; rec.distance = 0.0f;
		if (qi < d.n_live) {
			const GrassLive lv = d.live[qi];
			const GrassGroupDev g = d.groups[lv.group];
			const LmxGrassQuad q = d.quads[lv.slot];
			if (g.usable && q.instances_count != 0) { // :2140, :2161
				const DV3 tpos = DV3{d.terrain_pos[3 * g.terrain], d.terrain_pos[3 * g.terrain + 1], d.terrain_pos[3 * g.terrain + 2]};
				// cp.frustum.getRelative(tr.pos).intersectAABB(quad.aabb), geometry.cpp:121-149 / :78-96
				const V3 offset = to_v3(sub(DV3{v.f.origin[0], v.f.origin[1], v.f.origin[2]}, tpos));
				bool visible = true;
				for (int k = 0; k < 6; ++k) {
					const float dk = relative_plane_d(v.f, offset, k);
					const float bx = v.f.nx[k] > 0.0f ? q.aabb_max[0] : q.aabb_min[0];
					const float by = v.f.ny[k] > 0.0f ? q.aabb_max[1] : q.aabb_min[1];
					const float bz = v.f.nz[k] > 0.0f ? q.aabb_max[2] : q.aabb_min[2];
					const float dp = (v.f.nx[k] * bx) + (v.f.ny[k] * by) + (v.f.nz[k] * bz);
					if (dp < -dk) visible = false;
				}
				if (!visible) {
					++culled;
				} else {
					const V3 ref_lod_pos = to_v3(sub(DV3{v.viewport[0], v.viewport[1], v.viewport[2]}, tpos)); // :2136
					const float quad_size = g.spacing * 32;
					const float cx = (float)q.ij[0] * quad_size + quad_size * 0.5f, cz = (float)q.ij[1] * quad_size + quad_size * 0.5f; // :2168
					const float dx = cx - ref_lod_pos.x, dz = cz - ref_lod_pos.z;
					const float distance = sqrtf(dx * dx + dz * dz);
					const float half_range = g.distance * 0.5f * v.lod_multiplier;
					float c = distance - half_range; // clamp(distance - half_range, 0.f, half_range): minimum(maximum(value, min), max)
					c = c > 0.0f ? c : 0.0f;
					c = c < half_range ? c : half_range;
					float count_scale = 1 - c / half_range;
					count_scale *= count_scale;
					count_scale *= count_scale;
					const uint32_t count = u32_of((float)q.instances_count * count_scale); // :2176
					if (count == 0) {
						++culled;
					} else {
						draw = true;
						rec.slot = lv.slot; rec.terrain = g.terrain; rec.type = g.type; rec.instance_count = count; rec.distance = distance;
						instances += count;
					}
				}
			}
		}
		const unsigned long long mask = __ballot(draw);
		if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
		__syncthreads();
		uint32_t before = 0, total = 0;
		for (uint32_t w = 0; w < WAVES; ++w) {
			if (w < wave) before += s_wave[w];
			total += s_wave[w];
		}
		if (draw) out[base + before + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u))] = rec; // (< n_live <= draw_stride)
		base += total;
		__syncthreads(); // (s_wave is written again)
	}
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		culled += __shfl_xor(culled, m);
		instances += __shfl_xor(instances, m);
	}
	if (lane == 0) { s_sum[0][wave] = culled; s_sum[1][wave] = instances; }
	__syncthreads();
	if (tid == 0) {
		LmxGrassCounts c;
		c.draws = base; c.culled = 0; c.instances = 0; c.live = d.n_live;
		for (uint32_t w = 0; w < WAVES; ++w) { c.culled += s_sum[0][w]; c.instances += s_sum[1][w]; }
		d.counts[view] = c;
	}
}

} // namespace

hipError_t launch_grass_quads(hipStream_t s, const GrassQuadsDevice& d) {
	if (d.n_jobs == 0) return hipSuccess;
	hipLaunchKernelGGL(k_grass_quads, dim3(d.n_jobs), dim3(GRASS_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_grass_cull(hipStream_t s, const GrassCullDevice& d, uint32_t n_views) {
	if (n_views == 0) return hipSuccess;
	hipLaunchKernelGGL(k_grass_cull, dim3(n_views), dim3(GRASS_CULL_BLOCK), 0, s, d);
	return hipGetLastError();
}

} // namespace lmx
