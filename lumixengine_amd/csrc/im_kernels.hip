// im_kernels.hip — InstancedModel on the device: RenderModuleImpl::initInstancedModelGPUData (renderer/render_module.cpp:1285-1365) and
// PipelineImpl::encodeInstancedModels (renderer/pipeline.cpp:2449-2660) with its compute shader (data/shaders/instancing.hlsl: PASS0..3,
// UPDATE_LODS) for every model of a view in two launches. FMA-free (-ffp-contract=off); the shader's dot products are written out in
// HLSL's left-to-right order (a transcription: the order the reference's GPU compiler picks is its own).
#include "lmx_im.h"

#include <cfloat>

namespace lmx {

namespace {

__device__ __forceinline__ float im_min(float a, float b) { return a < b ? a : b; } // minimum(a, b), core/math.h:420-422
__device__ __forceinline__ float im_max(float a, float b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t pick4(uint32_t i, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
	return i == 0 ? a0 : i == 1 ? a1 : i == 2 ? a2 : a3;
}
__device__ __forceinline__ uint64_t pick4(uint32_t i, uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3) {
	return i == 0 ? a0 : i == 1 ? a1 : i == 2 ? a2 : a3;
}

// AABB::contains, core/geometry.cpp:540-548 (a NaN coordinate fails no test: such a point lies in the first cell)
__device__ __forceinline__ bool aabb_contains(const float* mn, const float* mx, float x, float y, float z) {
	if (mn[0] > x) return false;
	if (mn[1] > y) return false;
	if (mn[2] > z) return false;
	if (x > mx[0]) return false;
	if (y > mx[1]) return false;
	if (z > mx[2]) return false;
	return true;
}

// initInstancedModelGPUData for one model per block: grid AABB (addPoint = minCoords / maxCoords, a NaN coordinate never wins, so the
// partial boxes of the lanes are NaN-free and their reduction in any order gives the serial result up to the sign of a zero), the 16
// cells, then the count and a STABLE scatter in input order (per 1024-instance round: per-wave ballots per cell, the waves' counts through
// LDS, a running offset per cell). Instances no cell accepts follow the placed ones, in input order.
__global__ __launch_bounds__(IM_BUILD_BLOCK) void k_im_grid_build(const LmxImInstance* __restrict__ in, uint32_t n, ImArrays a, uint32_t first,
	ImGridDev* __restrict__ grid) {
	constexpr uint32_t WAVES = IM_BUILD_BLOCK / 64;
	__shared__ float s_red[6][WAVES];
	__shared__ float s_cmin[16][3], s_cmax[16][3];
	__shared__ uint32_t s_wave[WAVES][17];
	__shared__ uint32_t s_base[17], s_run[17];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint64_t lt = (1ull << lane) - 1ull;
	float mn0 = FLT_MAX, mn1 = FLT_MAX, mn2 = FLT_MAX, mx0 = -FLT_MAX, mx1 = -FLT_MAX, mx2 = -FLT_MAX;
	for (uint32_t i = tid; i < n; i += IM_BUILD_BLOCK) {
		const float4 r1 = reinterpret_cast<const float4*>(in + i)[1];
		mn0 = im_min(r1.x, mn0); mn1 = im_min(r1.y, mn1); mn2 = im_min(r1.z, mn2);
		mx0 = im_max(r1.x, mx0); mx1 = im_max(r1.y, mx1); mx2 = im_max(r1.z, mx2);
	}
	for (int off = 32; off > 0; off >>= 1) {
		mn0 = im_min(__shfl_xor(mn0, off), mn0); mn1 = im_min(__shfl_xor(mn1, off), mn1); mn2 = im_min(__shfl_xor(mn2, off), mn2);
		mx0 = im_max(__shfl_xor(mx0, off), mx0); mx1 = im_max(__shfl_xor(mx1, off), mx1); mx2 = im_max(__shfl_xor(mx2, off), mx2);
	}
	if (lane == 0) {
		s_red[0][wave] = mn0; s_red[1][wave] = mn1; s_red[2][wave] = mn2;
		s_red[3][wave] = mx0; s_red[4][wave] = mx1; s_red[5][wave] = mx2;
	}
	__syncthreads();
	if (tid < 16) {
		float g[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
		for (uint32_t w = 0; w < WAVES; ++w) {
			for (int k = 0; k < 3; ++k) g[k] = im_min(s_red[k][w], g[k]);
			for (int k = 3; k < 6; ++k) g[k] = im_max(s_red[k][w], g[k]);
		}
		// cells, render_module.cpp:1299-1314: cell_size = (max.xz - min.xz) * 0.25f, cell i + 4 j, then shrink(-0.01f) (geometry.cpp:639-642)
		const float csx = (g[3] - g[0]) * 0.25f, csz = (g[5] - g[2]) * 0.25f;
		const uint32_t i = tid & 3u, j = tid >> 2;
		const float cminx = g[0] + csx * (float)i, cminy = g[1], cminz = g[2] + csz * (float)j;
		const float cmaxx = cminx + csx, cmaxy = g[4], cmaxz = cminz + csz;
		const float sh = -0.01f;
		s_cmin[tid][0] = cminx + sh; s_cmin[tid][1] = cminy + sh; s_cmin[tid][2] = cminz + sh;
		s_cmax[tid][0] = cmaxx - sh; s_cmax[tid][1] = cmaxy - sh; s_cmax[tid][2] = cmaxz - sh;
		for (int k = 0; k < 3; ++k) {
			grid->cmin[tid][k] = s_cmin[tid][k];
			grid->cmax[tid][k] = s_cmax[tid][k];
		}
		if (tid == 0)
			for (int k = 0; k < 3; ++k) {
				grid->mn[k] = g[k];
				grid->mx[k] = g[3 + k];
			}
	}
	if (tid < 17) s_run[tid] = 0;
	__syncthreads();
	auto cell_of = [&](uint32_t i) -> uint32_t { // the FIRST cell whose AABB::contains accepts the point (16: none)
		const float4 r1 = reinterpret_cast<const float4*>(in + i)[1];
		uint32_t c = 16;
		for (uint32_t k = 0; k < 16; ++k)
			if (c == 16 && aabb_contains(s_cmin[k], s_cmax[k], r1.x, r1.y, r1.z)) c = k;
		return c;
	};
	// count (lane k < 17 of every wave keeps the wave's count of cell k)
	uint32_t my_count = 0;
	for (uint32_t base = 0; base < n; base += IM_BUILD_BLOCK) {
		const uint32_t i = base + tid;
		const uint32_t c = i < n ? cell_of(i) : 17u;
		for (uint32_t k = 0; k < 17; ++k) {
			const uint64_t m = __ballot(c == k);
			if (lane == k) my_count += (uint32_t)__popcll(m);
		}
	}
	if (lane < 17) s_wave[wave][lane] = my_count;
	__syncthreads();
	if (tid == 0) { // offsets, render_module.cpp:1326-1329; the unplaced instances start behind the last cell
		uint32_t at = 0;
		for (uint32_t c = 0; c < 17; ++c) {
			uint32_t total = 0;
			for (uint32_t w = 0; w < WAVES; ++w) total += s_wave[w][c];
			s_base[c] = at;
			if (c < 16) {
				grid->from[c] = at;
				grid->count[c] = total;
			}
			at += total;
		}
		grid->placed = s_base[16];
		grid->unplaced = at - s_base[16];
	}
	__syncthreads();
	// stable scatter, render_module.cpp:1333-1345
	for (uint32_t base = 0; base < n; base += IM_BUILD_BLOCK) {
		const uint32_t i = base + tid;
		const uint32_t c = i < n ? cell_of(i) : 17u;
		uint32_t rank = 0;
		for (uint32_t k = 0; k < 17; ++k) {
			const uint64_t m = __ballot(c == k);
			if (c == k) rank = (uint32_t)__popcll(m & lt);
			if (lane == k) s_wave[wave][k] = (uint32_t)__popcll(m);
		}
		__syncthreads();
		if (c < 17) {
			uint32_t dst = s_base[c] + s_run[c] + rank;
			for (uint32_t w = 0; w < wave; ++w) dst += s_wave[w][c];
			const float4* r = reinterpret_cast<const float4*>(in + i);
			const float4 r0 = r[0], r1 = r[1];
			const size_t g = (size_t)first + dst;
			a.pos_scale[g] = make_float4(r1.x, r1.y, r1.z, r1.w);
			a.rot[g] = make_float4(r0.x, r0.y, r0.z, 0.0f);
			a.lod[g] = r0.w;
		}
		__syncthreads();
		if (tid < 17) {
			uint32_t total = 0;
			for (uint32_t w = 0; w < WAVES; ++w) total += s_wave[w][tid];
			s_run[tid] += total;
		}
		__syncthreads();
	}
}

// The cell pass of encodeInstancedModels (pipeline.cpp:2507-2545) for one cell: 0 = skipped (empty or not near), 1 = near but not
// visible (UPDATE_LODS snaps), 2 = visible (PASS1 / PASS3).
__device__ __forceinline__ uint32_t cell_verdict(const ImViewDev& v, const ImModelDev& md, const ImGridDev& gd, uint32_t c) {
	if (gd.count[c] == 0) return 0;
	const DV3 origin = DV3{md.origin[0], md.origin[1], md.origin[2]};
	// view.cp.frustum.getRelative(origin.pos).intersectAABBWithOffset(cell.aabb, radius), geometry.cpp:121-149 / :58-75
	const V3 offset = to_v3(sub(DV3{v.f.origin[0], v.f.origin[1], v.f.origin[2]}, origin));
	const float* mn = gd.cmin[c];
	const float* mx = gd.cmax[c];
	bool visible = true;
	for (int k = 0; k < 6; ++k) {
		const float d = relative_plane_d(v.f, offset, k);
		const float bx = v.f.nx[k] > 0.0f ? mx[0] : mn[0];
		const float by = v.f.ny[k] > 0.0f ? mx[1] : mn[1];
		const float bz = v.f.nz[k] > 0.0f ? mx[2] : mn[2];
		const float dp = (v.f.nx[k] * bx) + (v.f.ny[k] * by) + (v.f.nz[k] * bz);
		if (dp < -d - md.radius) visible = false;
	}
	// length(origin.pos - view.cp.pos + cell_center) - cell_radius < draw_distance: DVec3 + Vec3 is a DVec3 (math.cpp:514), length fp64
	const V3 cmn = V3{mn[0], mn[1], mn[2]}, cmx = V3{mx[0], mx[1], mx[2]};
	const V3 center = mul(add(cmx, cmn), 0.5f);
	const V3 half = mul(sub(cmx, cmn), 0.5f);
	const float cell_radius = sqrtf(half.x * half.x + half.y * half.y + half.z * half.z);
	const DV3 rel = add(sub(origin, DV3{v.cam[0], v.cam[1], v.cam[2]}), center);
	const double len = sqrt(rel.x * rel.x + rel.y * rel.y + rel.z * rel.z);
	if (!(len - (double)cell_radius < (double)md.draw_distance)) return 0;
	return visible ? 2u : 1u;
}

struct ImLanePlan { // per block: what k_im_count and k_im_emit both derive from the model table
	uint32_t model, t0, n_it;
};
__device__ __forceinline__ ImLanePlan plan_of(const ImModelDev& md, uint32_t tile, uint32_t model) {
	ImLanePlan p;
	p.model = model;
	p.t0 = (tile - md.first_tile) * IM_TILE;
	p.n_it = md.n > p.t0 ? min((md.n - p.t0 + IM_BLOCK - 1) / IM_BLOCK, IM_TILE / IM_BLOCK) : 0u;
	return p;
}

// instancing.hlsl cull(): dot(u_camera_planes[i], float4(p, 1)) < -u_radius * scale culls (a NaN passes every plane)
__device__ __forceinline__ bool sphere_passes(const DevFrustum& f, float px, float py, float pz, float scaled_radius) {
	bool pass = true;
	for (int k = 0; k < 6; ++k) {
		const float dp = ((f.nx[k] * px + f.ny[k] * py) + f.nz[k] * pz) + f.d[k];
		if (dp < -scaled_radius) pass = false;
	}
	return pass;
}

__device__ __forceinline__ uint32_t lod_bin(float lod) { return lod > 0.0f ? (uint32_t)lod : 0u; } // uint(lod): v_cvt_u32_f32 saturates

// PASS1 (+ UPDATE_LODS) for one tile of one model: the block's 16 cell verdicts, then per instance the LOD update of non-shadow views
// (cross-fade in visible cells, snap to the target in near-but-invisible cells), the sphere test of visible cells and the bins it feeds.
// Out: the tile's four bin counts and one emission bit per instance (64-bit word per wave and round), read by k_im_emit instead of the
// instance records.
__global__ __launch_bounds__(IM_BLOCK) void k_im_count(const ImModelDev* __restrict__ models, const ImGridDev* __restrict__ grids,
	const uint32_t* __restrict__ tile_model, ImViewDev v, ImArrays a, uint64_t* __restrict__ masks, uint4* __restrict__ tile_counts, uint32_t* __restrict__ model_tot) {
	__shared__ uint32_t s_verdict[16], s_end[16];
	__shared__ uint32_t s_bins[IM_BLOCK / 64][4];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
	const uint32_t m = tile_model[tile];
	const ImModelDev& md = models[m];
	const ImGridDev& gd = grids[m];
	const ImLanePlan p = plan_of(md, tile, m);
	if (tid < 16) {
		s_verdict[tid] = cell_verdict(v, md, gd, tid);
		s_end[tid] = gd.from[tid] + gd.count[tid];
	}
	__syncthreads();
	// camera_offset = Vec3(origin.pos - view.cp.pos); lod_distances * multiplier, below 0 -> FLT_MAX (pipeline.cpp:2547-2551)
	const V3 co = to_v3(sub(DV3{md.origin[0], md.origin[1], md.origin[2]}, DV3{v.cam[0], v.cam[1], v.cam[2]}));
	float ld[4];
	for (int k = 0; k < 4; ++k) {
		ld[k] = md.lod_dist[k] * v.lod_multiplier;
		if (ld[k] < 0) ld[k] = FLT_MAX;
	}
	const float td = v.time_delta * 2;
	const uint32_t placed = gd.placed;
	// block-uniform: a tile none of whose instances lies in a near cell does nothing (no load, no LOD store, no mask: k_im_emit skips it)
	bool active = false;
	for (int k = 0; k < 16; ++k) {
		const uint32_t from = k ? s_end[k - 1] : 0u;
		active = active || (s_verdict[k] != 0 && from < s_end[k] && from < p.t0 + IM_TILE && s_end[k] > p.t0);
	}
	const uint32_t n_it = active ? p.n_it : 0u;
	uint32_t bc0 = 0, bc1 = 0, bc2 = 0, bc3 = 0;
	for (uint32_t it = 0; it < n_it; ++it) {
		const uint32_t li = p.t0 + it * IM_BLOCK + tid; // instance index inside the model
		const size_t g = (size_t)md.first + li;
		bool emit = false;
		uint32_t b0 = 0;
		bool two = false;
		if (li < placed) {
			uint32_t c = 0;
			for (int k = 0; k < 16; ++k) c += s_end[k] <= li ? 1u : 0u;
			const uint32_t verdict = s_verdict[c];
			if (verdict) {
				const float4 ps = a.pos_scale[g];
				const float px = ps.x + co.x, py = ps.y + co.y, pz = ps.z + co.z;
				float lod = 0;
				if (!v.is_shadow) { // getLOD: d = dot(p, p)
					const float d = (px * px + py * py) + pz * pz;
					const float dst = d > ld[3] ? 4.0f : d > ld[2] ? 3.0f : d > ld[1] ? 2.0f : d > ld[0] ? 1.0f : 0.0f;
					if (verdict == 1) {
						lod = dst;
					} else { // cross-fade: lod = |d| < td ? dst : src + td * sign(d)
						const float src = a.lod[g];
						const float dd = dst - src;
						const float sgn = (float)((dd > 0.0f ? 1 : 0) - (dd < 0.0f ? 1 : 0));
						lod = fabsf(dd) < td ? dst : src + td * sgn;
					}
					a.lod[g] = lod;
				} else if (verdict == 2) {
					lod = a.lod[g];
				}
				if (verdict == 2 && lod <= 3.0f && sphere_passes(v.f, px, py, pz, md.radius * ps.w)) {
					emit = true;
					b0 = lod_bin(lod);
					two = lod - floorf(lod) > 0.01f;
				}
			}
		}
		const uint64_t mask = __ballot(emit);
		if (lane == 0 && p.t0 + it * IM_BLOCK + wave * 64 < md.n) masks[((size_t)md.first + p.t0 + it * IM_BLOCK + wave * 64) >> 6] = mask;
		bc0 += (uint32_t)__popcll(__ballot(emit && b0 == 0));
		bc1 += (uint32_t)__popcll(__ballot(emit && (b0 == 1 || (two && b0 == 0))));
		bc2 += (uint32_t)__popcll(__ballot(emit && (b0 == 2 || (two && b0 == 1))));
		bc3 += (uint32_t)__popcll(__ballot(emit && (b0 == 3 || (two && b0 == 2))));
	}
	if (lane == 0) {
		s_bins[wave][0] = bc0; s_bins[wave][1] = bc1; s_bins[wave][2] = bc2; s_bins[wave][3] = bc3;
	}
	__syncthreads();
	if (tid == 0) {
		uint4 t = make_uint4(0, 0, 0, 0);
		for (uint32_t w = 0; w < IM_BLOCK / 64; ++w) {
			t.x += s_bins[w][0]; t.y += s_bins[w][1]; t.z += s_bins[w][2]; t.w += s_bins[w][3];
		}
		tile_counts[tile] = t;
		if (t.x | t.y | t.z | t.w) { // the model's bin totals (sums: the order of the adds does not matter)
			atomicAdd(model_tot + 4 * m + 0, t.x);
			atomicAdd(model_tot + 4 * m + 1, t.y);
			atomicAdd(model_tot + 4 * m + 2, t.z);
			atomicAdd(model_tot + 4 * m + 3, t.w);
		}
	}
}

// PASS0 / PASS2 / PASS3 for one tile: the bin offsets (the model's base = the bin totals k_im_count summed for the models before it, bin b
// of the model behind bins 0..b-1, this tile behind the model's earlier tiles), the model's indirect records and counts (its first tile),
// then the records in ascending instance order: per round the waves' per-bin counts through LDS. Block 0 also clears the totals the NEXT
// run's k_im_count adds into (model_tot_next: the other half of a double buffer), so a run needs no fill.
__global__ __launch_bounds__(IM_BLOCK) void k_im_emit(const ImModelDev* __restrict__ models, const ImGridDev* __restrict__ grids,
	const uint32_t* __restrict__ tile_model, ImViewDev v, ImArrays a, const uint32_t* __restrict__ indices_count, const uint64_t* __restrict__ masks,
	const uint4* __restrict__ tile_counts, const uint32_t* __restrict__ model_tot, uint32_t* __restrict__ model_tot_next, LmxImInstance* __restrict__ records,
	LmxImIndirect* __restrict__ indirect, ImCountsDev* __restrict__ counts) {
	__shared__ uint32_t s_red[9][IM_BLOCK / 64];
	__shared__ uint32_t s_w[2][IM_BLOCK / 64][4];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
	const uint64_t lt = (1ull << lane) - 1ull;
	const uint32_t m = tile_model[tile];
	const ImModelDev& md = models[m];
	const ImLanePlan p = plan_of(md, tile, m);
	const uint32_t mt0 = md.first_tile;
	if (tile == 0)
		for (uint32_t k = tid; k < 4 * v.n_models; k += IM_BLOCK) model_tot_next[k] = 0;
	const uint4 mine = tile_counts[tile];
	const bool drawn = (mine.x | mine.y | mine.z | mine.w) != 0;
	if (tile != mt0 && !drawn) return; // block-uniform: nothing of this tile is drawn and it writes no per-model record
	uint32_t r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // base, model totals[4], tile prefix[4]
	for (uint32_t k = tid; k < m; k += IM_BLOCK) r[0] += (model_tot[4 * k] + model_tot[4 * k + 1]) + (model_tot[4 * k + 2] + model_tot[4 * k + 3]);
	if (drawn)
		for (uint32_t k = mt0 + tid; k < tile; k += IM_BLOCK) {
			const uint4 c = tile_counts[k];
			r[5] += c.x; r[6] += c.y; r[7] += c.z; r[8] += c.w;
		}
	for (int j = 0; j < 9; ++j) {
		if (j >= 1 && j <= 4) continue;
		for (int off = 32; off > 0; off >>= 1) r[j] += __shfl_xor(r[j], off);
		if (lane == 0) s_red[j][wave] = r[j];
	}
	__syncthreads();
	for (int j = 0; j < 9; ++j) {
		if (j >= 1 && j <= 4) continue;
		uint32_t t = 0;
		for (uint32_t w = 0; w < IM_BLOCK / 64; ++w) t += s_red[j][w];
		r[j] = t;
	}
	for (int j = 0; j < 4; ++j) r[1 + j] = model_tot[4 * m + j];
	const uint32_t off0 = r[0], off1 = off0 + r[1], off2 = off1 + r[2], off3 = off2 + r[3];
	if (tile == mt0) {
		if (tid == 0) {
			ImCountsDev c;
			c.bin_count[0] = r[1]; c.bin_count[1] = r[2]; c.bin_count[2] = r[3]; c.bin_count[3] = r[4];
			c.bin_offset[0] = off0; c.bin_offset[1] = off1; c.bin_offset[2] = off2; c.bin_offset[3] = off3;
			c.indirect_offset = md.indirect_offset;
			c.mesh_count = md.mesh_count;
			c.instances = md.n;
			c.unplaced = grids[m].unplaced;
			counts[m] = c;
		}
		if (tid < md.mesh_count) { // PASS2: meshes up to lod_indices.w draw their LOD's bin; the model's other slots draw nothing
			const int32_t i = (int32_t)tid;
			LmxImIndirect rec;
			rec.vertex_count = indices_count[md.indirect_offset + tid];
			rec.first_index = 0;
			rec.base_vertex = 0;
			rec.instance_count = 0;
			rec.base_instance = 0;
			if (i <= md.lod_idx[3]) {
				const uint32_t b = i <= md.lod_idx[0] ? 0u : i <= md.lod_idx[1] ? 1u : i <= md.lod_idx[2] ? 2u : 3u;
				rec.instance_count = pick4(b, r[1], r[2], r[3], r[4]);
				rec.base_instance = pick4(b, off0, off1, off2, off3);
			}
			indirect[md.indirect_offset + tid] = rec;
		}
	}
	if (!drawn) return;
	const V3 co = to_v3(sub(DV3{md.origin[0], md.origin[1], md.origin[2]}, DV3{v.cam[0], v.cam[1], v.cam[2]}));
	uint32_t run0 = off0 + r[5], run1 = off1 + r[6], run2 = off2 + r[7], run3 = off3 + r[8];
	for (uint32_t it = 0; it < p.n_it; ++it) {
		const uint32_t li = p.t0 + it * IM_BLOCK + tid;
		const size_t g = (size_t)md.first + li;
		const uint32_t group = p.t0 + it * IM_BLOCK + wave * 64;
		const uint64_t word = group < md.n ? masks[((size_t)md.first + group) >> 6] : 0ull;
		const bool emit = (word >> lane) & 1ull;
		float4 ps = make_float4(0, 0, 0, 0), rt = make_float4(0, 0, 0, 0);
		float lod = 0;
		if (emit) {
			lod = a.lod[g];
			ps = a.pos_scale[g];
			rt = a.rot[g];
		}
		const uint32_t b0 = lod_bin(lod);
		const float t = lod - floorf(lod);
		const bool two = emit && t > 0.01f;
		const uint64_t m0 = __ballot(emit && b0 == 0);
		const uint64_t m1 = __ballot((emit && b0 == 1) || (two && b0 == 0));
		const uint64_t m2 = __ballot((emit && b0 == 2) || (two && b0 == 1));
		const uint64_t m3 = __ballot((emit && b0 == 3) || (two && b0 == 2));
		const uint32_t par = it & 1u;
		if (lane == 0) {
			s_w[par][wave][0] = (uint32_t)__popcll(m0); s_w[par][wave][1] = (uint32_t)__popcll(m1);
			s_w[par][wave][2] = (uint32_t)__popcll(m2); s_w[par][wave][3] = (uint32_t)__popcll(m3);
		}
		__syncthreads();
		uint32_t pre0 = 0, pre1 = 0, pre2 = 0, pre3 = 0, tot0 = 0, tot1 = 0, tot2 = 0, tot3 = 0;
		for (uint32_t w = 0; w < IM_BLOCK / 64; ++w) {
			const uint32_t c0 = s_w[par][w][0], c1 = s_w[par][w][1], c2 = s_w[par][w][2], c3 = s_w[par][w][3];
			if (w < wave) {
				pre0 += c0; pre1 += c1; pre2 += c2; pre3 += c3;
			}
			tot0 += c0; tot1 += c1; tot2 += c2; tot3 += c3;
		}
		if (emit) { // PASS3: (rot.xyz, w, pos_scale + (camera_offset, 0))
			const float4 q = make_float4(ps.x + co.x, ps.y + co.y, ps.z + co.z, ps.w + 0.0f);
			{
				const uint32_t at = pick4(b0, run0 + pre0, run1 + pre1, run2 + pre2, run3 + pre3) + (uint32_t)__popcll(pick4(b0, m0, m1, m2, m3) & lt);
				float4* o = reinterpret_cast<float4*>(records + at);
				o[0] = make_float4(rt.x, rt.y, rt.z, t);
				o[1] = q;
			}
			if (two) {
				const uint32_t b1 = b0 + 1;
				const uint32_t at = pick4(b1, run0 + pre0, run1 + pre1, run2 + pre2, run3 + pre3) + (uint32_t)__popcll(pick4(b1, m0, m1, m2, m3) & lt);
				float4* o = reinterpret_cast<float4*>(records + at);
				o[0] = make_float4(rt.x, rt.y, rt.z, t - 1.0f);
				o[1] = q;
			}
		}
		run0 += tot0; run1 += tot1; run2 += tot2; run3 += tot3;
	}
}

} // namespace

hipError_t launch_im_grid_build(hipStream_t s, const LmxImInstance* in, uint32_t n, ImArrays a, uint32_t first, ImGridDev* grid) {
	hipLaunchKernelGGL(k_im_grid_build, dim3(1), dim3(IM_BUILD_BLOCK), 0, s, in, n, a, first, grid);
	return hipGetLastError();
}

hipError_t launch_im_run(hipStream_t s, const ImModelDev* models, const ImGridDev* grids, const uint32_t* tile_model, uint32_t n_tiles, const ImViewDev& view,
	ImArrays a, const uint32_t* indices_count, uint64_t* masks, uint4* tile_counts, uint32_t* model_tot, uint32_t* model_tot_next, LmxImInstance* records,
	LmxImIndirect* indirect, ImCountsDev* counts) {
	if (!n_tiles) return hipSuccess;
	hipLaunchKernelGGL(k_im_count, dim3(n_tiles), dim3(IM_BLOCK), 0, s, models, grids, tile_model, view, a, masks, tile_counts, model_tot);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_im_emit, dim3(n_tiles), dim3(IM_BLOCK), 0, s, models, grids, tile_model, view, a, indices_count, masks, tile_counts, model_tot, model_tot_next, records, indirect,
		counts);
	return hipGetLastError();
}

} // namespace lmx
