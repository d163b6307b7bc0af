// voxel_kernels.hip — Voxels (renderer/voxels.cpp) on the device: raster, computeAO, blurAO and the point lookups. The arithmetic is
// lmx_voxels.h's, shared with the host; FMA-free (-ffp-contract=off), so voxel bytes, AO floats and baked u8 values equal the reference's.
//
//   k_voxel_raster  ONE WAVE per (triangle, part). The wave computes the triangle's cell box cut to the grid (a set of cells: what lies
//                   outside is skipped by setVoxel anyway), its lanes stride the box's cells and test each with testAABBTriangleCollision;
//                   a hit stores the byte 1 (plain vector store; several waves may store the same 1). gridDim.y parts share a large box:
//                   part p takes the cells p * 64 + lane, + 64 * parts, ...
//   k_voxel_ao      The rays of the whole grid are one sequence: ray g = voxel * ray_count + d draws the generator's values 3 g .. 3 g + 2.
//                   A wave takes a run of whole voxels and walks its rays in chunks of 64, one ray per lane. A lane reaches its first state
//                   by the closed form (voxel_rng_skip) and every further one by a multiplication with a^192 mod m: 64 rays on. The hits of
//                   a chunk are one ballot; the voxels that end inside the chunk get their count from its bits (a voxel may span chunks:
//                   the count carries over) and their AO as `hits` subtractions, run redundantly by every lane, stored by lane 0.
//                   LDS = true: the block first packs the grid's bytes into a bit mask in LDS (VOXEL_AO_LDS_WORDS words) and the march
//                   reads that; LDS = false: the march reads the bytes in global memory (grids over 32 * VOXEL_AO_LDS_WORDS cells).
//   k_voxel_blur    one lane per voxel: 27 clamped samples in c (z), b (y), a (x) order, sequential adds, / 9.f.
//   k_voxel_sample  one lane per point: the cell of voxel_point_cell, then the voxel byte, the AO or the importer's u8.
#include <hip/hip_runtime.h>

#include "lmx_voxels.h"

namespace lmx {

namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t WAVES = VOXEL_BLOCK / WAVE;
// a^192 mod m: 64 rays of three draws each
constexpr uint64_t pow_mod(uint64_t a, uint64_t k, uint64_t m) {
	uint64_t r = 1;
	for (a %= m; k; k >>= 1) {
		if (k & 1) r = r * a % m;
		a = a * a % m;
	}
	return r;
}
constexpr uint32_t A192_U = (uint32_t)pow_mod(VOXEL_RNG_A_U, 192, VOXEL_RNG_M_U);
constexpr uint32_t A192_V = (uint32_t)pow_mod(VOXEL_RNG_A_V, 192, VOXEL_RNG_M_V);

__global__ __launch_bounds__(VOXEL_BLOCK) void k_voxel_raster(VoxelGrid g, const float* __restrict__ tris, uint32_t n_tris, uint8_t* __restrict__ voxels) {
	const uint32_t t = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (t >= n_tris) return;
	const float* p = tris + 9 * (size_t)t;
	const V3 a = V3{p[0], p[1], p[2]}, b = V3{p[3], p[4], p[5]}, c = V3{p[6], p[7], p[8]};
	const VoxelSpan s = voxel_clip_box(g, voxel_triangle_box(g, a, b, c));
	const uint64_t stride = (uint64_t)WAVE * gridDim.y;
	for (uint64_t cell = (uint64_t)blockIdx.y * WAVE + lane; cell < s.n; cell += stride) { // s.n <= the grid's cells < 2^31
		const uint32_t cc = (uint32_t)cell;
		const uint32_t ci = cc % s.ext[0], rest = cc / s.ext[0];
		const int32_t i = s.lo[0] + (int32_t)ci, j = s.lo[1] + (int32_t)(rest % s.ext[1]), k = s.lo[2] + (int32_t)(rest / s.ext[1]);
		if (voxel_cell_hits_triangle(g, i, j, k, a, b, c)) voxels[(size_t)i + (size_t)j * g.res[0] + (size_t)k * ((size_t)g.res[0] * g.res[1])] = 1; // in the grid: the span was cut to it
	}
}

// bit k = byte k of x is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
	const uint32_t t = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
	return (t | t >> 7 | t >> 14 | t >> 21) & 0xfu;
}

// one lane's generator at ray `ray` of the sequence, 64 rays behind its last one where it had one
__device__ __forceinline__ VoxelRng ao_rng_at(VoxelRng seed, VoxelRng prev, uint64_t ray, bool first) {
	// the state 3 * ray draws behind the seed is canonical from two draws on: only ray 0 starts at the seed itself, and steps on by the closed form
	if (first || ray < 65) return voxel_rng_skip(seed, 3 * ray);
	return VoxelRng{voxel_rng_mul<VOXEL_RNG_M_U>(prev.u, A192_U), voxel_rng_mul<VOXEL_RNG_M_V>(prev.v, A192_V)};
}

template <bool LDS> __global__ __launch_bounds__(VOXEL_BLOCK) void k_voxel_ao(VoxelGrid g, const uint8_t* __restrict__ voxels, uint32_t n_cells, uint32_t ray_count, VoxelRng seed,
	uint32_t voxels_per_wave, float* __restrict__ ao) {
	__shared__ uint32_t s_mask[LDS ? VOXEL_AO_LDS_WORDS : 1];
	if (LDS) {
		const uint32_t n_words = (n_cells + 31u) / 32u; // <= VOXEL_AO_LDS_WORDS: checked by the launcher
		for (uint32_t w = threadIdx.x; w < n_words; w += VOXEL_BLOCK) {
			uint32_t bits = 0;
			const uint32_t at = w * 32u;
			if (n_cells - at >= 32u) { // 32 bytes in two 16-byte loads (the grid's buffer is an allocation of its own: 32 w is aligned)
				const uint4* src = reinterpret_cast<const uint4*>(voxels + at);
				const uint4 q0 = src[0], q1 = src[1];
				bits = nonzero_bytes(q0.x) | nonzero_bytes(q0.y) << 4 | nonzero_bytes(q0.z) << 8 | nonzero_bytes(q0.w) << 12 | nonzero_bytes(q1.x) << 16 | nonzero_bytes(q1.y) << 20 |
					nonzero_bytes(q1.z) << 24 | nonzero_bytes(q1.w) << 28;
			} else {
				for (uint32_t k = 0; k < n_cells - at; ++k) bits |= (voxels[at + k] ? 1u : 0u) << k;
			}
			s_mask[w] = bits;
		}
		__syncthreads();
	}
	const uint32_t wave = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	const uint64_t first_voxel = (uint64_t)wave * voxels_per_wave;
	if (first_voxel >= n_cells) return; // (behind the barrier; whole waves leave)
	const uint64_t end_voxel = first_voxel + voxels_per_wave < n_cells ? first_voxel + voxels_per_wave : n_cells;
	const uint64_t ray_end = end_voxel * ray_count;
	uint64_t voxel = first_voxel; // the voxel whose rays the chunk's first ray belongs to
	uint32_t hits = 0;            // of `voxel`, in the chunks before this one
	VoxelRng rng = seed;
	bool first = true;
	for (uint64_t chunk = first_voxel * ray_count; chunk < ray_end; chunk += WAVE) {
		const uint64_t ray = chunk + lane;
		rng = ao_rng_at(seed, rng, ray, first); // every lane keeps its state up to date, also past the end: no lane depends on another's
		first = false;
		bool hit = false;
		if (ray < ray_end) {
			const uint32_t v = (uint32_t)(ray / ray_count);
			const int32_t x = (int32_t)(v % (uint32_t)g.res[0]), yz = (int32_t)(v / (uint32_t)g.res[0]);
			const int32_t y = yz % g.res[1], z = yz / g.res[1];
			VoxelRng draw = rng;
			const V3 dir = voxel_ray_dir(draw);
			if (LDS) hit = voxel_cast_ray(g, x, y, z, dir, [&](uint32_t idx) { return (s_mask[idx >> 5] >> (idx & 31u)) & 1u; });
			else hit = voxel_cast_ray(g, x, y, z, dir, [&](uint32_t idx) { return voxels[idx]; });
		}
		const uint64_t mask = __ballot(hit);
		const uint64_t chunk_end = chunk + WAVE < ray_end ? chunk + WAVE : ray_end;
		uint64_t pos = chunk;
		while (pos < chunk_end) { // wave-uniform: the voxels with rays in this chunk
			const uint64_t voxel_end = (voxel + 1) * ray_count;
			const uint64_t seg_end = voxel_end < chunk_end ? voxel_end : chunk_end;
			const uint32_t lo = (uint32_t)(pos - chunk), n = (uint32_t)(seg_end - pos); // 1 <= n <= 64
			const uint64_t bits = (mask >> lo) & (n == 64 ? ~0ull : (1ull << n) - 1ull);
			hits += (uint32_t)__popcll(bits);
			if (seg_end == voxel_end) {
				const float value = voxel_ao_of_hits(hits, ray_count);
				if (lane == 0) ao[voxel] = value;
				hits = 0;
				++voxel;
			}
			pos = seg_end;
		}
	}
}

__global__ __launch_bounds__(VOXEL_BLOCK) void k_voxel_blur(VoxelGrid g, uint32_t n_cells, const float* __restrict__ ao, float* __restrict__ blurred) {
	const uint32_t idx = blockIdx.x * VOXEL_BLOCK + threadIdx.x;
	if (idx >= n_cells) return;
	const int32_t rx = g.res[0], ry = g.res[1], rz = g.res[2];
	const int32_t x = (int32_t)(idx % (uint32_t)rx), yz = (int32_t)(idx / (uint32_t)rx);
	const int32_t y = yz % ry, z = yz / ry;
	float v = 0;
	for (int32_t c = -1; c <= 1; ++c) {
		const int32_t zz = z + c < 0 ? 0 : (z + c > rz - 1 ? rz - 1 : z + c);
		for (int32_t b = -1; b <= 1; ++b) {
			const int32_t yy = y + b < 0 ? 0 : (y + b > ry - 1 ? ry - 1 : y + b);
			for (int32_t a = -1; a <= 1; ++a) {
				const int32_t xx = x + a < 0 ? 0 : (x + a > rx - 1 ? rx - 1 : x + a);
				v += ao[voxel_index(g, xx, yy, zz)];
			}
		}
	}
	blurred[idx] = v / 9.f;
}

__global__ __launch_bounds__(VOXEL_BLOCK) void k_voxel_sample(VoxelGrid g, int mode, const uint8_t* __restrict__ voxels, const float* __restrict__ ao, const float* __restrict__ points,
	uint32_t n, float min_ao, uint8_t* __restrict__ out_u8, float* __restrict__ out_f, uint8_t* __restrict__ inside) {
	const uint32_t i = blockIdx.x * VOXEL_BLOCK + threadIdx.x;
	if (i >= n) return;
	const V3 p = V3{points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
	uint32_t idx = 0;
	const bool in = voxel_point_cell(g, p, &idx);
	inside[i] = in ? 1 : 0;
	if (!in) return;
	if (mode == VOXEL_SAMPLE_VOXEL) out_u8[i] = voxels[idx];
	else if (mode == VOXEL_SAMPLE_AO) out_f[i] = ao[idx];
	else out_u8[i] = voxel_bake_u8(ao[idx], min_ao);
}

} // namespace

hipError_t launch_voxel_raster(hipStream_t s, const VoxelGrid& g, const float* tris, uint32_t n_tris, uint32_t split, uint8_t* voxels) {
	if (n_tris == 0 || voxel_cells(g) == 0) return hipSuccess;
	if (split < 1) split = 1;
	if (split > VOXEL_RASTER_MAX_SPLIT) split = VOXEL_RASTER_MAX_SPLIT;
	hipLaunchKernelGGL(k_voxel_raster, dim3((n_tris + WAVES - 1) / WAVES, split), dim3(VOXEL_BLOCK), 0, s, g, tris, n_tris, voxels);
	return hipGetLastError();
}

hipError_t launch_voxel_ao(hipStream_t s, const VoxelGrid& g, const uint8_t* voxels, uint32_t ray_count, VoxelRng seed, float* ao, bool lds) {
	const uint64_t cells = voxel_cells(g);
	if (cells == 0) return hipSuccess;
	if (cells > 0x7fffffffull || ray_count == 0) return hipErrorInvalidValue;
	const uint32_t n_cells = (uint32_t)cells;
	// whole voxels per wave, VOXEL_AO_CHUNKS_PER_WAVE chunks of 64 rays or more: the lanes' closed-form start is paid once per wave
	uint64_t per_wave = ((uint64_t)VOXEL_AO_CHUNKS_PER_WAVE * WAVE + ray_count - 1) / ray_count;
	if (per_wave < 1) per_wave = 1;
	if (per_wave > n_cells) per_wave = n_cells;
	const uint32_t voxels_per_wave = (uint32_t)per_wave;
	const uint32_t n_waves = (uint32_t)((cells + voxels_per_wave - 1) / voxels_per_wave);
	const dim3 grid((n_waves + WAVES - 1) / WAVES);
	if (lds && cells <= 32ull * VOXEL_AO_LDS_WORDS) hipLaunchKernelGGL(k_voxel_ao<true>, grid, dim3(VOXEL_BLOCK), 0, s, g, voxels, n_cells, ray_count, seed, voxels_per_wave, ao);
	else hipLaunchKernelGGL(k_voxel_ao<false>, grid, dim3(VOXEL_BLOCK), 0, s, g, voxels, n_cells, ray_count, seed, voxels_per_wave, ao);
	return hipGetLastError();
}

hipError_t launch_voxel_blur(hipStream_t s, const VoxelGrid& g, const float* ao, float* blurred) {
	const uint64_t cells = voxel_cells(g);
	if (cells == 0) return hipSuccess;
	if (cells > 0x7fffffffull) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_voxel_blur, dim3((uint32_t)((cells + VOXEL_BLOCK - 1) / VOXEL_BLOCK)), dim3(VOXEL_BLOCK), 0, s, g, (uint32_t)cells, ao, blurred);
	return hipGetLastError();
}

hipError_t launch_voxel_sample(hipStream_t s, const VoxelGrid& g, int mode, const uint8_t* voxels, const float* ao, const float* points, uint32_t n, float min_ao, uint8_t* out_u8,
	float* out_f, uint8_t* inside) {
	if (n == 0) return hipSuccess;
	hipLaunchKernelGGL(k_voxel_sample, dim3((n + VOXEL_BLOCK - 1) / VOXEL_BLOCK), dim3(VOXEL_BLOCK), 0, s, g, mode, voxels, ao, points, n, min_ao, out_u8, out_f, inside);
	return hipGetLastError();
}

} // namespace lmx
