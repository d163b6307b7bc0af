// ray_scene_kernels.hip — the rest of RenderModuleImpl::castRay (renderer/render_module.cpp:2715-2780) behind the stages of ray_kernels.hip:
// castRayProceduralGeometry (:2650-2712), Terrain::castRay (renderer/terrain.cpp:474-535) with both getHeight (:402-447), and the merge of
// :2761-2775 into one record per ray. FMA-free (-ffp-contract=off), fp32 with IEEE divisions; the one fp64 step per pair is origin - position.
//
//   k_pgray_broad    (256-geometry tile x ray tile) pairs, stepped as k_imray_broad steps its pairs: one geometry per thread in registers (the
//                    entity's transform, the AABB), the rays staged in LDS. ro = Vec3(tr.invTransform(origin)), rd = tr.invTransformVector(dir)
//                    NOT normalised (:2665-2666), the gate aabb.contains(ro) || getRayAABBIntersection (:2669). A survivor becomes a
//                    RayCandidate on the shared list: entity = model = the geometry's index, never a palette.
//   k_ray_narrow     of ray_kernels.hip, unchanged: the RaysDevice it is handed points at this stage's own model / mesh / position / index
//                    tables (one one-mesh model per geometry; a non-indexed geometry got an implicit 32-bit index list at the upload).
//   k_pgray_resolve  per candidate with a hit: the winning triangle's own t (tested once more: the cell holds -0 as +0) - rd is not normalised,
//                    so it is the world parameter the reference compares (:2700, :2762) - and the ray's minimum over ordered float bits.
//   k_pgray_write    LmxRayPgHit: zero for a ray without a hit, the winner's for the others; the stage's counters; bit 2 of the entity
//                    stage's overflow word.
//   k_terrain_ray    ONE WAVE per (ray, terrain) pair. The walk's cell sequence is serial in floating point (next_x += delta_x accumulates
//                    its roundings), so every lane runs the cheap recurrence and lane l keeps the state of step 64 k + l of chunk k; each lane
//                    then interpolates the four corner heights of its own cell and tests its two triangles. A ballot picks the first lane
//                    with a hit, triangle (p0, p1, p2) ahead of (p0, p2, p3) within it; the wave stops at the first chunk with a hit or with
//                    the walk's end. That is the reference's "first cell along the walk, first triangle of the cell", not the nearest hit.
//   k_ray_scene_write  castRay's result: the model-instance hit, else the instanced-model hit, then the procedural hit and every terrain in
//                    table order as :2762 and :2769-2773 compare them.
#include "lmx_kernels.h"
#include "lmx_entity_tr.h"
#include "lmx_ray_math.h"
#include "lmx_wave.h"
#include "lmx_terrain_height.h" // both Terrain::getHeight, shared with grass_kernels.hip

namespace lmx {

namespace {

constexpr unsigned long long RAY_NONE = ~0ull;
constexpr uint32_t WAVE = 64;
static_assert(RAY_TERRAIN_CHUNK == WAVE && RAY_BLOCK % WAVE == 0, "one step of a chunk per lane");

// the filter of castRay(ray, ignored), :2603-2607: `hit.entity != ignored || !ignored.isValid()`
__device__ __forceinline__ bool refused(const LmxRay& ray, int32_t entity) { return ray.ignore >= 0 && entity == ray.ignore; }

// ---- procedural geometry ----

__global__ __launch_bounds__(RAY_BLOCK) void k_pgray_broad(SceneRaysDevice q) {
	__shared__ LmxRay s_rays[RAY_BROAD_RAYS];
	const RaysDevice& d = q.r;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_rt = (d.n_rays + RAY_BROAD_RAYS - 1) / RAY_BROAD_RAYS;
	const uint32_t n_gt = (q.n_pg + RAY_BLOCK - 1) / RAY_BLOCK;
	if (n_rt == 0) return;
	// pair p = gt * n_rt + rt for p = blockIdx.x, + RAY_PG_BROAD_GRID, ...: kept as (gt, rt), stepped as in k_ray_broad
	const uint32_t gt_step = RAY_PG_BROAD_GRID / n_rt, rt_step = RAY_PG_BROAD_GRID % n_rt;
	uint32_t cur_gt = 0xffffffffu;
	// the thread's geometry
	bool ok = false;
	uint32_t g = 0;
	int32_t entity = 0;
	DV3 pos = {};
	Q4 rot = {};
	V3 inv_scale = {}, mn = {}, mx_box = {}, mx = {};
	uint32_t rt = blockIdx.x % n_rt;
	for (uint32_t gt = blockIdx.x / n_rt; gt < n_gt; gt += gt_step) {
		if (rt >= n_rt) { // (the carry of the step before)
			rt -= n_rt;
			if (++gt >= n_gt) break;
		}
		if (gt != cur_gt) {
			cur_gt = gt;
			g = gt * RAY_BLOCK + threadIdx.x;
			ok = false;
			if (g < q.n_pg && q.pg[g].castable) { // `vertex_data.empty()` / `primitive_type != TRIANGLES`, :2655-2656
				ok = true;
				entity = q.pg[g].entity;
				const DrawTr t = load_tr(d, (uint32_t)entity);
				pos = DV3{t.px, t.py, t.pz};
				rot = Q4{__uint_as_float(t.rot[0]), __uint_as_float(t.rot[1]), __uint_as_float(t.rot[2]), __uint_as_float(t.rot[3])};
				inv_scale = V3{safe_inverse_scale(__uint_as_float(t.scale[0])), safe_inverse_scale(__uint_as_float(t.scale[1])), safe_inverse_scale(__uint_as_float(t.scale[2]))};
				const RayModelRec& mo = d.models[g];
				mn = V3{mo.aabb_min[0], mo.aabb_min[1], mo.aabb_min[2]};
				mx_box = V3{mo.aabb_max[0], mo.aabb_max[1], mo.aabb_max[2]};
				mx = add(mn, sub(mx_box, mn)); // min + size with size = aabb.max - aabb.min, :2669
			}
		}
		__syncthreads(); // (the previous tile's rays are no longer read)
		const uint32_t ray0 = rt * RAY_BROAD_RAYS;
		const uint32_t n_tile = d.n_rays - ray0 < RAY_BROAD_RAYS ? d.n_rays - ray0 : RAY_BROAD_RAYS;
		if (threadIdx.x < n_tile) s_rays[threadIdx.x] = d.rays[ray0 + threadIdx.x];
		__syncthreads();
		for (uint32_t r = 0; r < n_tile; ++r) { // (block-uniform: every lane takes every ballot)
			const LmxRay& ray = s_rays[r];
			bool pass = ok && !refused(ray, entity); // the filter would refuse every triangle of the geometry (:2703-2705)
			V3 ro = {}, rd = {};
			if (pass) {
				const Q4 conj = conjugated(rot);
				const V3 rv = rotate(conj, V3{ray.dir[0], ray.dir[1], ray.dir[2]}); // invTransformVector, math.cpp:789-797
				rd = V3{rv.x * inv_scale.x, rv.y * inv_scale.y, rv.z * inv_scale.z};
				const DV3 rotated = rotate(conj, sub(DV3{ray.origin[0], ray.origin[1], ray.origin[2]}, pos)); // Transform::invTransform(DVec3), math.cpp:767-774
				ro = to_v3(DV3{rotated.x * inv_scale.x, rotated.y * inv_scale.y, rotated.z * inv_scale.z});
				// AABB::contains, core/geometry.cpp:540-548
				const bool contains = !(mn.x > ro.x) && !(mn.y > ro.y) && !(mn.z > ro.z) && !(ro.x > mx_box.x) && !(ro.y > mx_box.y) && !(ro.z > mx_box.z);
				float tmin;
				pass = contains || ray_aabb_tmin(ro, rd, mn, mx, &tmin);
			}
			const unsigned long long mask = __ballot(pass); // (written out, lane 0 leads: see k_ray_broad, ray_kernels.hip)
			if (mask == 0) continue; // (wave-uniform)
			unsigned long long base = 0;
			if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long*>(d.state + RAYS_COUNTER), (unsigned long long)__popcll(mask));
			base = __shfl(base, 0);
			const unsigned long long at = base + rank_in(mask);
			if (pass && at < d.max_cand) {
				RayCandidate c;
				c.ray = ray0 + r; c.entity = g;
				c.o[0] = ro.x; c.o[1] = ro.y; c.o[2] = ro.z;
				c.d[0] = rd.x; c.d[1] = rd.y; c.d[2] = rd.z;
				c.model = g; c.palette_at = RAY_NO_PALETTE; c.n_bones = 0; c.pad = 0;
				d.cand[at] = c;
				d.cand_best[at] = RAY_NONE;
			}
		}
		rt += rt_step; // (< 2 n_rt)
	}
}

// the winning triangle's own t (the cell holds -0 as +0): the same loads and the same arithmetic as the narrow phase give the same bits
__device__ __forceinline__ float pg_winner(const RaysDevice& d, const RayCandidate& cd, unsigned long long best) {
	const RayMeshRec& me = d.meshes[d.models[cd.model].first_mesh];
	const uint32_t tri = (uint32_t)best;
	V3 p[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t i = 3 * tri + k;
		const uint32_t v = me.index_bytes == 2 ? reinterpret_cast<const uint16_t*>(d.indices + me.index_at)[i] : reinterpret_cast<const uint32_t*>(d.indices + me.index_at)[i];
		const float* c = d.positions + 3 * ((size_t)me.vert_at + v); // (v < n_verts: checked when the table was set)
		p[k] = V3{c[0], c[1], c[2]};
	}
	float t = __uint_as_float((uint32_t)(best >> 32));
	ray_triangle(p[0], p[1], p[2], V3{cd.o[0], cd.o[1], cd.o[2]}, V3{cd.d[0], cd.d[1], cd.d[2]}, &t);
	return t;
}

__global__ __launch_bounds__(RAY_BLOCK) void k_pgray_resolve(SceneRaysDevice q) {
	const RaysDevice& d = q.r;
	const uint32_t n_cand = candidates(d);
	for (uint32_t c = blockIdx.x * RAY_BLOCK + threadIdx.x; c < n_cand; c += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const unsigned long long best = d.cand_best[c];
		if (best == RAY_NONE) continue;
		const RayCandidate cd = d.cand[c];
		const float t = pg_winner(d, cd, best);
		d.cand_t[c] = t;
		atomicMin(&q.pg_best[cd.ray], ordered_key(t, cd.entity)); // (never a NaN: ray_triangle refuses it)
	}
}

__global__ __launch_bounds__(RAY_BLOCK) void k_pgray_write(SceneRaysDevice q) {
	const RaysDevice& d = q.r;
	const uint32_t n_cand = candidates(d);
	const uint32_t gid = blockIdx.x * RAY_BLOCK + threadIdx.x;
	for (uint32_t r = gid; r < d.n_rays; r += RAY_RESOLVE_GRID * RAY_BLOCK) {
		if (q.pg_best[r] != RAY_NONE) continue; // (a candidate below writes it)
		LmxRayPgHit h;
		h.is_hit = 0; h.entity = 0; h.geom = 0; h.triangle = 0; h.t = 0.0f;
		q.pg_hits[r] = h;
	}
	for (uint32_t c = gid; c < n_cand; c += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const unsigned long long best = d.cand_best[c];
		if (best == RAY_NONE) continue;
		const RayCandidate cd = d.cand[c];
		const float t = d.cand_t[c];
		if (q.pg_best[cd.ray] != ordered_key(t, cd.entity)) continue; // (one candidate per (ray, geometry): one winner)
		LmxRayPgHit h;
		h.is_hit = 1; h.entity = q.pg[cd.entity].entity; h.geom = cd.entity; h.triangle = (uint32_t)best; h.t = t;
		q.pg_hits[cd.ray] = h;
	}
	if (gid == 0) {
		const unsigned long long n = *reinterpret_cast<const unsigned long long*>(d.state + RAYS_COUNTER);
		d.state[RAYS_CANDIDATES] = n < 0xffffffffull ? (uint32_t)n : 0xffffffffu;
		d.state[RAYS_OVERFLOW] = n > d.max_cand ? 1u : 0u;
		if (n > d.max_cand) q.entity_state[RAYS_OVERFLOW] |= RAYS_PG_OVERFLOW; // (k_ray_write has finished: the launches are in stream order)
	}
}

// ---- terrain ----

__device__ __forceinline__ float abs_of(float v) { return __uint_as_float(__float_as_uint(v) & 0x7fffffffu); } // fabsf

__global__ __launch_bounds__(RAY_BLOCK) void k_terrain_ray(SceneRaysDevice q) {
	const RaysDevice& d = q.r;
	const uint32_t lane = threadIdx.x & 63u;
	if (q.n_terrains == 0) return;
	// pair p = r * n_terrains + k for p = the wave's index, + n_waves, ...: kept as (r, k) and stepped without a 64-bit division, as the broad phases step
	constexpr uint32_t n_waves = RAY_TERRAIN_GRID * (RAY_BLOCK / WAVE);
	static_assert(RAY_MAX_TERRAINS <= n_waves, "r_step > 0");
	const uint32_t r_step = n_waves / q.n_terrains, k_step = n_waves % q.n_terrains;
	const uint32_t first = blockIdx.x * (RAY_BLOCK / WAVE) + threadIdx.x / WAVE;
	uint32_t k = first % q.n_terrains;
	for (uint32_t r = first / q.n_terrains; r < d.n_rays; r += r_step, k += k_step) {
		if (k >= q.n_terrains) { // (the carry of the step before)
			k -= q.n_terrains;
			if (++r >= d.n_rays) break;
		}
		// (everything up to the cell test is wave-uniform: the pair is)
		const unsigned long long p = (unsigned long long)r * q.n_terrains + k;
		const RayTerrainRec& te = q.terrains[k];
		LmxRayTerrainHit out;
		out.is_hit = 0; out.entity = 0; out.terrain = 0; out.hx = 0; out.hz = 0; out.tri = 0; out.t = 0.0f;
		bool walk = te.ready != 0; // `!m_heightmap || !m_heightmap->isReady()`, :479
		TerrainView tv = {};
		V3 rel = {}, dir = {};
		int32_t hx = 0, hz = 0, step_x = 0, step_z = 0;
		float next_x = 0, next_z = 0, delta_x = 0, delta_z = 0;
		if (walk) {
			tv.texels = q.texels + te.texel_at; tv.w = (int32_t)te.width; tv.h = (int32_t)te.height; tv.format = te.format;
			tv.sx = te.scale[0]; tv.sy = te.scale[1]; tv.sz = te.scale[2];
			const LmxRay& ray = d.rays[r];
			const DrawTr t = load_tr(d, (uint32_t)te.entity); // world.getPosition(m_entity), :482: rotation and scale are not read
			rel = to_v3(sub(DV3{ray.origin[0], ray.origin[1], ray.origin[2]}, DV3{t.px, t.py, t.pz}));
			dir = V3{ray.dir[0], ray.dir[1], ray.dir[2]};
			const V3 size = V3{(float)tv.w * tv.sx, tv.sy * 65535.0f, (float)tv.h * tv.sx};
			float tmin = 0;
			walk = ray_aabb_tmin(rel, dir, V3{0.0f, 0.0f, 0.0f}, add(V3{0.0f, 0.0f, 0.0f}, size), &tmin);
			if (walk) {
				const V3 start = tmin < 0 ? rel : add(rel, mul(dir, tmin));
				hx = trunc_i32f(start.x / tv.sx);
				hz = trunc_i32f(start.z / tv.sx);
				const bool flat_x = abs_of(dir.x) < 0.01f, flat_z = abs_of(dir.z) < 0.01f;
				// (flat: the cell index itself, as the reference really does, :492-493)
				next_x = flat_x ? (float)hx : ((float)(hx + (dir.x < 0 ? 0 : 1)) * tv.sx - rel.x) / dir.x;
				next_z = flat_z ? (float)hz : ((float)(hz + (dir.z < 0 ? 0 : 1)) * tv.sx - rel.z) / dir.z;
				delta_x = flat_x ? 0.0f : tv.sx / abs_of(dir.x);
				delta_z = flat_z ? 0.0f : tv.sz / abs_of(dir.z); // (scale.z, :496; every other place reads scale.x)
				step_x = dir.x > 0 ? 1 : (dir.x < 0 ? -1 : 0);
				step_z = dir.z > 0 ? 1 : (dir.z < 0 ? -1 : 0);
			}
		}
		const uint32_t bound = te.width + te.height; // every walk that ends moves hx or hz by one per iteration: it ends within this many
		bool ended = !walk, found = false;
		for (uint32_t s0 = 0; !ended && !found; s0 += RAY_TERRAIN_CHUNK) {
			// the recurrence, on every lane alike; lane l keeps the cell of step s0 + l
			int32_t my_hx = 0, my_hz = 0;
			bool mine = false;
			for (uint32_t i = 0; i < RAY_TERRAIN_CHUNK; ++i) {
				if (!(s0 + i < bound && hx >= 0 && hz >= 0 && (long long)hx + step_x < tv.w && (long long)hz + step_z < tv.h)) { // :500
					ended = true;
					break;
				}
				if (i == lane) { my_hx = hx; my_hz = hz; mine = true; }
				if (next_x < next_z && step_x != 0) { // :522
					next_x += delta_x;
					hx += step_x;
				} else {
					if (step_z == 0) ended = true; // DEVIATION: nothing changes from here on; the reference never returns
					next_z += delta_z;
					hz += step_z;
				}
				if (delta_x == 0 && delta_z == 0) ended = true; // :530
				if (ended) break;
			}
			bool hit = false;
			uint32_t tri = 0;
			float t = 0;
			if (mine) { // :502-521
				const float x = (float)my_hx * tv.sx, z = (float)my_hz * tv.sx;
				const float x1 = x + tv.sx, z1 = z + tv.sx;
				const V3 p0 = V3{x, terrain_height(tv, x, z), z};
				const V3 p1 = V3{x1, terrain_height(tv, x1, z), z};
				const V3 p2 = V3{x1, terrain_height(tv, x1, z1), z1};
				const V3 p3 = V3{x, terrain_height(tv, x, z1), z1};
				hit = ray_triangle(p0, p1, p2, rel, dir, &t);
				if (!hit) {
					hit = ray_triangle(p0, p2, p3, rel, dir, &t);
					tri = 1;
				}
			}
			const unsigned long long mask = __ballot(hit); // (the loop's condition is wave-uniform: every lane is here)
			found = mask != 0;
			if (found && lane == (uint32_t)__ffsll((long long)mask) - 1u) { // the first cell along the walk, whatever its t
				out.is_hit = 1; out.entity = te.entity; out.terrain = k; out.hx = my_hx; out.hz = my_hz; out.tri = tri; out.t = t;
				q.terrain_hits[p] = out;
			}
		}
		if (!found && lane == 0) q.terrain_hits[p] = out; // (the all-zero record)
	}
}

// ---- castRay's result ----

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_scene_write(SceneRaysDevice q) {
	const RaysDevice& d = q.r;
	const uint32_t gid = blockIdx.x * RAY_BLOCK + threadIdx.x;
	for (uint32_t r = gid; r < d.n_rays; r += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const LmxRay& ray = d.rays[r];
		LmxRaySceneHit hit;
		hit.is_hit = 0; hit.component = 0; hit.entity = 0; hit.index = 0; hit.sub = 0; hit.t = 0.0f;
		const LmxRayHit h = q.hits[r];
		if (h.is_hit) { // (nearer than the instanced-model hit: the entity stage cast with that hit's t as t_max, :2746)
			hit.is_hit = 1; hit.component = LMX_RAY_HIT_MODEL_INSTANCE; hit.entity = h.entity; hit.index = h.mesh; hit.sub = h.triangle; hit.t = h.t;
		} else if (q.im_hits && q.im_hits[r].is_hit) {
			const LmxRayImHit ih = q.im_hits[r];
			hit.is_hit = 1; hit.component = LMX_RAY_HIT_INSTANCED_MODEL; hit.entity = ih.entity; hit.index = ih.model; hit.sub = ih.subindex; hit.t = ih.t;
		}
		const LmxRayPgHit pg = q.pg_hits[r];
		if (pg.is_hit && pg.t < ray.t_max && (pg.t < hit.t || !hit.is_hit)) { // :2762; t_max: the hit the caller holds
			hit.is_hit = 1; hit.component = LMX_RAY_HIT_PROCEDURAL_GEOM; hit.entity = pg.entity; hit.index = pg.geom; hit.sub = pg.triangle; hit.t = pg.t;
		}
		for (uint32_t k = 0; k < q.n_terrains; ++k) { // :2767-2775, the filter at the merge (:2773)
			const LmxRayTerrainHit th = q.terrain_hits[(unsigned long long)r * q.n_terrains + k];
			if (th.is_hit && th.t < ray.t_max && (!hit.is_hit || th.t < hit.t) && !refused(ray, th.entity)) {
				hit.is_hit = 1; hit.component = LMX_RAY_HIT_TERRAIN; hit.entity = th.entity; hit.index = k; hit.sub = (uint32_t)th.hz * q.terrains[k].width + (uint32_t)th.hx; hit.t = th.t;
			}
		}
		q.scene_hits[r] = hit;
	}
	if (gid == 0) d.state[RAYS_RAYS] = d.n_rays;
}

} // namespace

hipError_t launch_pgrays_broad(hipStream_t s, const SceneRaysDevice& d) {
	hipLaunchKernelGGL(k_pgray_broad, dim3(RAY_PG_BROAD_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_pgrays_resolve(hipStream_t s, const SceneRaysDevice& d) {
	hipLaunchKernelGGL(k_pgray_resolve, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_pgray_write, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_terrain_rays(hipStream_t s, const SceneRaysDevice& d) {
	hipLaunchKernelGGL(k_terrain_ray, dim3(RAY_TERRAIN_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_scene_write(hipStream_t s, const SceneRaysDevice& d) {
	hipLaunchKernelGGL(k_ray_scene_write, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

} // namespace lmx
