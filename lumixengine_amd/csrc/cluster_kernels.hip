// cluster_kernels.hip — PipelineImpl::fillClusters (renderer/pipeline.cpp:3327-3684) on the device: the listed lights become ClusterLight
// records (:3387-3410), the enabled probes their records (:3500-3531), and lights and probes are binned into the view's cluster grid with
// range() of :3540-3561 - `clusters` {offset, lights_count, env_probes_count, refl_probes_count} and `map`, a cluster's segment holding its
// light indices ascending, then its environment probe indices, then its reflection probe indices (the reference's three sequential fill
// passes, :3649-3662). FMA-free (-ffp-contract=off); the fp64 subtract + convert of Vec3(pos - cam_pos) is the only fp64 work.
//
// The list and its length stay on the device: every launch has a FIXED grid, nothing is sized from a read-back. Four launches:
//   k_cluster_records  per listed light the 64-byte record (the first max_lights of them) and its cluster range on the three axes, packed
//                      into 8 bytes; the blocks behind CLUSTER_REC_GRID do the same for the probes. The view's planes arrive as a kernel
//                      argument (built on the host with libm's powf, lmx_cluster_planes.cpp) and are staged in LDS.
//   k_cluster_count    a cluster-side GATHER: each wave owns a cluster, its block stages the packed ranges of CLUSTER_BLOCK lights at a time
//                      in LDS and every wave tests 64 of them per step against its cluster (ballot + popcount).
//   k_cluster_offsets  one block: the exclusive sum of the clusters' sizes in index order x + y * size.x + z * size.x * size.y, saturating
//                      at 2^32 - 1, and the counters. (No atomics anywhere: a counter is one store.)
//   k_cluster_fill     the same walk as the count: a hit's place in its cluster's segment is the hits before it (mbcnt of the ballot + the
//                      steps before) - ascending light order without a sort, the same from run to run. A segment that would pass
//                      map_capacity is not written.
#include "lmx_kernels.h"
#include "lmx_entity_tr.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

constexpr uint32_t CLUSTER_WAVES = CLUSTER_BLOCK / 64;
constexpr uint32_t PLANES_X = 0, PLANES_Y = 65, PLANES_Z = 130;

// planeDist, core/geometry.cpp:826-828
__device__ __forceinline__ float plane_dist(float4 pl, float x, float y, float z) { return ((pl.x * x + pl.y * y) + pl.z * z) + pl.w; }

// range() of :3540-3561 over planes[0 .. size], as (lo + 1) | (hi + 1) << 8. The reference's early returns as one loop every lane walks
// in step (the planes are LDS broadcasts): plane 0 decides "behind everything"; the first plane i + 1 the sphere is not beyond (dist > r
// is false) gives lo = i; from that same plane on the first one it lies wholly behind (dist < -r) gives hi; else hi = size. The
// comparisons are the reference's, so a NaN distance fails every one of them: lo = 0, hi = size.
__device__ __forceinline__ uint32_t axis_range(const float4* planes, int size, float x, float y, float z, float r) {
	int lo = -1, hi = -1;
	bool done = plane_dist(planes[0], x, y, z) < -r;
	for (int k = 1; k <= size; ++k) {
		const float dist = plane_dist(planes[k], x, y, z);
		if (!done) {
			if (lo < 0 && !(dist > r)) lo = k - 1;
			if (lo >= 0 && dist < -r) {
				hi = k;
				done = true;
			}
		}
	}
	if (!done && lo >= 0) hi = size;
	return (uint32_t)(lo + 1) | (uint32_t)(hi + 1) << 8;
}

__device__ __forceinline__ uint2 cluster_ranges(const ClustersDevice& d, const float4* s_planes, float x, float y, float z, float r) {
	const uint32_t rx = axis_range(s_planes + PLANES_X, (int)d.size_x, x, y, z, r);
	const uint32_t ry = axis_range(s_planes + PLANES_Y, (int)d.size_y, x, y, z, r);
	const uint32_t rz = axis_range(s_planes + PLANES_Z, (int)d.size_z, x, y, z, r);
	return make_uint2(rx | ry << 16, rz);
}

// cluster (cx, cy, cz) + 1 on every axis against a packed range: lo <= c < hi on all three (an axis that came out (-1, -1) holds nothing)
__device__ __forceinline__ bool in_ranges(uint2 r, uint32_t cx1, uint32_t cy1, uint32_t cz1) {
	return cx1 >= (r.x & 0xffu) && cx1 < ((r.x >> 8) & 0xffu) && cy1 >= ((r.x >> 16) & 0xffu) && cy1 < (r.x >> 24) && cz1 >= (r.y & 0xffu) && cz1 < ((r.y >> 8) & 0xffu);
}

__device__ __forceinline__ float rel_f32(double p, double cam) { return (float)(p - cam); } // Vec3(pos - cam_pos), one component

// Step 1.
__global__ __launch_bounds__(CLUSTER_BLOCK) void k_cluster_records(ClustersDevice d, ClusterPlanesArg p) {
	__shared__ float4 s_planes[CLUSTER_N_PLANES];
	for (uint32_t k = threadIdx.x; k < CLUSTER_N_PLANES; k += CLUSTER_BLOCK) s_planes[k] = p.planes[k];
	__syncthreads();
	if (blockIdx.x >= CLUSTER_REC_GRID) { // the probes (:3500-3531), already in output order
		const uint32_t n_probes = d.n_env + d.n_refl;
		for (uint32_t j = (blockIdx.x - CLUSTER_REC_GRID) * CLUSTER_BLOCK + threadIdx.x; j < n_probes; j += CLUSTER_PROBE_BLOCKS * CLUSTER_BLOCK) {
			const bool env = j < d.n_env;
			const uint32_t k = env ? j : j - d.n_env;
			const int32_t e = env ? d.env_entity[k] : d.refl_entity[k];
			const DrawTr t = load_tr(d, (uint32_t)e);
			const float x = rel_f32(t.px, d.cam[0]), y = rel_f32(t.py, d.cam[1]), z = rel_f32(t.pz, d.cam[2]);
			const float4 rot = make_float4(__uint_as_float(t.rot[0]), __uint_as_float(t.rot[1]), __uint_as_float(t.rot[2]), -__uint_as_float(t.rot[3])); // conjugated(): core/math.cpp:664-667
			if (env) {
				const ClusterEnvRec& in = d.env_tmpl[k];
				ClusterEnvRec& out = d.env_out[k];
				out.v[0] = make_float4(x, y, z, 0.0f);
				out.v[1] = rot;
				for (int q = 2; q < 13; ++q) out.v[q] = in.v[q];
			} else {
				const ClusterReflRec& in = d.refl_tmpl[k];
				ClusterReflRec& out = d.refl_out[k];
				out.v[0] = make_float4(x, y, z, in.v[0].w); // layer
				out.v[1] = rot;
				out.v[2] = in.v[2];
			}
			d.probe_ranges[j] = cluster_ranges(d, s_planes, x, y, z, env ? d.env_radius[k] : d.refl_radius[k]);
		}
		return;
	}
	const uint32_t n = list_length(d);
	for (uint32_t i = blockIdx.x * CLUSTER_BLOCK + threadIdx.x; i < n; i += CLUSTER_REC_GRID * CLUSTER_BLOCK) { // (list_cap <= 2^30: no wrap)
		const int32_t e = d.list[i];
		const uint32_t ue = (uint32_t)e; // a negative entity lies past every table
		const DrawTr t = load_tr(d, ue);
		const float x = rel_f32(t.px, d.cam[0]), y = rel_f32(t.py, d.cam[1]), z = rel_f32(t.pz, d.cam[2]);
		float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q = c; // {color, intensity} {range, fov, attenuation_param, flags}
		if (ue < d.n_light_tab) {
			const float4* rec = reinterpret_cast<const float4*>(d.light_tab + ue);
			c = rec[0];
			q = rec[1];
		}
		if (i < d.max_lights) {
			uint32_t atlas = 0xffffffffu;
			if (d.atlas) atlas = ue < d.n_atlas ? d.atlas[ue] : 0u;
			float4* out = d.lights + (size_t)i * 4;
			out[0] = make_float4(x, y, z, q.x);                                       // pos, radius
			out[1] = make_float4(__uint_as_float(t.rot[0]), __uint_as_float(t.rot[1]), __uint_as_float(t.rot[2]), __uint_as_float(t.rot[3]));
			out[2] = make_float4(c.x * c.w, c.y * c.w, c.z * c.w, q.z);               // color * intensity, attenuation_param
			out[3] = make_float4(__uint_as_float(atlas), q.y, 0.0f, 0.0f);            // atlas_idx, fov, padding
			d.light_entities[i] = e;
		}
		d.ranges[i] = cluster_ranges(d, s_planes, x, y, z, q.x);
	}
}

// One tile of packed ranges against the block's clusters: the wave's hits among `n_items` items, counted - and, FILL, their indices written
// to map[at ..) in ascending order. Every thread of the block takes every barrier.
template <bool FILL> __device__ __forceinline__ uint32_t gather(const uint2* items, uint32_t n_items, uint2* s_r, bool valid, uint32_t cx1, uint32_t cy1, uint32_t cz1, int32_t* map, uint32_t at, uint32_t map_capacity) {
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t count = 0;
	for (uint32_t base = 0; base < n_items; base += CLUSTER_BLOCK) {
		const uint32_t i = base + threadIdx.x;
		s_r[threadIdx.x] = i < n_items ? items[i] : make_uint2(0u, 0u);
		__syncthreads();
		for (uint32_t sub = 0; sub < CLUSTER_WAVES && base + sub * 64 < n_items; ++sub) { // (block-uniform bounds)
			const bool hit = valid && in_ranges(s_r[sub * 64 + lane], cx1, cy1, cz1);
			const unsigned long long mask = __ballot(hit);
			if (FILL) {
				const uint32_t to = at + count + rank_in(mask); // (< offset + total <= map_capacity: the count step saw the same ranges)
				if (hit && to < map_capacity) map[to] = (int32_t)(base + sub * 64 + lane);
			}
			count += (uint32_t)__popcll(mask);
		}
		__syncthreads();
	}
	return count;
}

// Steps 2 and 4.
template <bool FILL> __global__ __launch_bounds__(CLUSTER_BLOCK) void k_cluster_gather(ClustersDevice d) {
	__shared__ uint2 s_r[CLUSTER_BLOCK];
	const uint32_t n = list_length(d);
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t per_z = d.size_x * d.size_y;
	for (uint32_t cbase = blockIdx.x * CLUSTER_WAVES; cbase < d.n_clusters; cbase += CLUSTER_GRID * CLUSTER_WAVES) {
		const uint32_t c = cbase + wave;
		const bool valid = c < d.n_clusters;
		const uint32_t cz = c / per_z, in_z = c - cz * per_z, cy = in_z / d.size_x, cx = in_z - cy * d.size_x;
		uint32_t at = 0;
		bool fits = false;
		if (FILL && valid) { // a segment that would pass the map's end is not written: nothing behind it fits either
			const uint32_t offset = d.offsets[c];
			fits = (uint64_t)offset + d.totals[c] <= d.map_capacity;
			at = offset;
		}
		const bool take = FILL ? fits : valid;
		const uint32_t nl = gather<FILL>(d.ranges, n, s_r, take, cx + 1, cy + 1, cz + 1, d.map, at, d.map_capacity);
		const uint32_t ne = gather<FILL>(d.probe_ranges, d.n_env, s_r, take, cx + 1, cy + 1, cz + 1, d.map, at + nl, d.map_capacity);
		const uint32_t nr = gather<FILL>(d.probe_ranges + d.n_env, d.n_refl, s_r, take, cx + 1, cy + 1, cz + 1, d.map, at + nl + ne, d.map_capacity);
		if (!FILL && valid && lane == 0) {
			d.clusters[c] = make_uint4(0u, nl, ne, nr);
			d.totals[c] = nl + ne + nr; // (<= 2^30 + 2048)
		}
	}
}

// Step 3. Thread t owns the clusters [t * per, (t + 1) * per).
__global__ __launch_bounds__(CLUSTER_SCAN_BLOCK) void k_cluster_offsets(ClustersDevice d) {
	__shared__ uint32_t s_wave[CLUSTER_SCAN_BLOCK / 64];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t per = (d.n_clusters + CLUSTER_SCAN_BLOCK - 1) / CLUSTER_SCAN_BLOCK;
	const uint32_t begin = tid * per < d.n_clusters ? tid * per : d.n_clusters, end = begin + per < d.n_clusters ? begin + per : d.n_clusters;
	uint32_t sum = 0;
	for (uint32_t c = begin; c < end; ++c) sum = sat_add(sum, d.totals[c]);
	// lmx_wave.h's block_scan<true> written out WITHOUT its trailing barrier (s_wave is not used again): with the barrier this one-block
	// kernel took 15.26-15.27 us against 14.96-15.03 us (tools/cluster_time.py under a kernel trace, profiles/wave/README.md)
	const uint32_t v = wave_inclusive(sum, lane, SatAdd());
	if (lane == 63) s_wave[wave] = v;
	__syncthreads();
	uint32_t before = 0, all = 0;
	for (uint32_t w = 0; w < CLUSTER_SCAN_BLOCK / 64; ++w) {
		const uint32_t sw = s_wave[w];
		if (w < wave) before = sat_add(before, sw);
		all = sat_add(all, sw);
	}
	uint32_t ex = __shfl_up(v, 1u); // (saturating sums: the exclusive value is the inclusive one of the lane before, not v - sum)
	if (lane == 0) ex = 0;
	uint32_t offset = sat_add(before, ex);
	for (uint32_t c = begin; c < end; ++c) {
		d.offsets[c] = offset;
		reinterpret_cast<uint32_t*>(d.clusters + c)[0] = offset;
		offset = sat_add(offset, d.totals[c]);
	}
	if (tid == 0) {
		const uint32_t n_listed = list_length(d);
		d.state[CLUSTERS_LIGHTS] = n_listed;
		d.state[CLUSTERS_ENV] = d.n_env;
		d.state[CLUSTERS_REFL] = d.n_refl;
		d.state[CLUSTERS_MAP] = all;
		d.state[CLUSTERS_OVERFLOW] = (n_listed > d.max_lights ? 1u : 0u) | (all > d.map_capacity ? 2u : 0u);
	}
}

} // namespace

hipError_t launch_cluster_records(hipStream_t s, const ClustersDevice& d, const ClusterPlanesArg& p) {
	hipLaunchKernelGGL(k_cluster_records, dim3(CLUSTER_REC_GRID + CLUSTER_PROBE_BLOCKS), dim3(CLUSTER_BLOCK), 0, s, d, p);
	return hipGetLastError();
}

hipError_t launch_cluster_bins(hipStream_t s, const ClustersDevice& d) {
	hipLaunchKernelGGL(k_cluster_gather<false>, dim3(CLUSTER_GRID), dim3(CLUSTER_BLOCK), 0, s, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_cluster_offsets, dim3(1), dim3(CLUSTER_SCAN_BLOCK), 0, s, d);
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_cluster_gather<true>, dim3(CLUSTER_GRID), dim3(CLUSTER_BLOCK), 0, s, d);
	return hipGetLastError();
}

} // namespace lmx
