// ray_kernels.hip — RenderModuleImpl::castRay's model-instance loop (renderer/render_module.cpp:2715-2759) with Model::castRay
// (renderer/model.cpp:139-223) for a batch of rays, on the device. FMA-free (-ffp-contract=off); fp32 and fp64 where the reference uses them.
//
// The reference walks the instances one after another and prunes against the nearest hit so far; the device result is the ORDER-FREE
// minimum: per ray the entity of smallest world-space t (ties: smallest entity), per entity the triangle of smallest model-space t (ties:
// first in (mesh, triangle) walk order). Both are 64-bit atomic minima of (t bits << 32) | index: for t >= 0 the bit pattern of a float
// is monotone once -0 is canonicalised. A NaN t is no hit. Every launch has a FIXED grid; nothing is sized from a read-back.
//   k_ray_broad    (entity tile x ray tile) pairs: one entity per thread in registers, RAY_BROAD_RAYS rays staged in LDS; flags, ignore,
//                  distance gate (:2729-2731), model-space ray (:2733-2734), sphere (:2737) and AABB (:2740). A survivor becomes a
//                  RayCandidate, appended with one returning atomic per wave and ray (ballot + mbcnt). The list's order is arbitrary.
//   k_ray_narrow   RAY_NARROW_SPLIT blocks share a candidate; a thread takes runs of RAY_RUN consecutive triangles of the model's LOD 0,
//                  chunk by chunk. A skinned candidate's palette is staged in LDS first (evaluateSkin, model.cpp:103-109). The wave's
//                  minimum goes to the candidate's cell with at most one atomic per wave.
//   k_ray_resolve  per candidate with a hit: the winning triangle's own t (it is tested once more: the cell holds -0 as +0), the hit
//                  position back in world space, new_t (:2743-2745), the ray's minimum.
//   k_ray_write    the hit records: zero for a ray without a hit, the winner's for the others; the counters.
//
// RenderModuleImpl::castRayInstancedModels (render_module.cpp:2609-2648) runs AHEAD of them over the attached instanced models, with the same
// candidate list, narrow phase and scratch, one stage after the other:
//   k_imray_broad   (256-slot instance tile x ray tile) pairs: one instance per thread in registers (pos_scale, rot, radius), the rays and
//                   `base` = Vec3(ray.origin - tr.pos) of the tile's model staged in LDS; the `ignore` filter, rel_pos (:2628), the sphere
//                   (:2631), the instance-space ray (:2632-2634). A survivor becomes a RayCandidate: entity = the global slot, pad = the
//                   lmx_im model, never a palette (the pose is null).
//   k_ray_narrow    unchanged, on that list.
//   k_imray_resolve per candidate with a hit: the triangle's own t, t * scale (:2636), the ray's minimum over ordered float bits (a negative
//                   scale gives negative products).
//   k_imray_write   the LmxRayImHit records, the rays with their effective t_max (the instanced-model hit's t, else the ray's own: `cur_dist`
//                   of :2719 and `new_t < hit.t` of :2746) for the stage above, the counters.
#include "lmx_kernels.h"
#include "lmx_entity_tr.h"
#include "lmx_im.h"
#include "lmx_ray_math.h"
#include "lmx_skin_eval.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

constexpr unsigned long long RAY_NONE = ~0ull;
constexpr uint32_t RAY_CHUNK = RAY_BLOCK * RAY_RUN; // triangles a block takes per step
enum : uint32_t { INSTANCE_ENABLED = 1u << 1, INSTANCE_VALID = 1u << 2 }; // ModelInstance::Flags, render_module.h:209-212

__device__ __forceinline__ double length_d(DV3 v) { return sqrt(v.x * v.x + v.y * v.y + v.z * v.z); } // core/math.cpp:393

struct RayTr { DV3 pos; Q4 rot; V3 scale; };
template <typename D> __device__ __forceinline__ RayTr load_ray_tr(const D& d, uint32_t e) {
	const DrawTr t = load_tr(d, e);
	RayTr r;
	r.pos = DV3{t.px, t.py, t.pz};
	r.rot = Q4{__uint_as_float(t.rot[0]), __uint_as_float(t.rot[1]), __uint_as_float(t.rot[2]), __uint_as_float(t.rot[3])};
	r.scale = V3{__uint_as_float(t.scale[0]), __uint_as_float(t.scale[1]), __uint_as_float(t.scale[2])};
	return r;
}

// getRaySphereIntersection(origin, dir, Vec3::ZERO, radius, t) && t >= 0, core/geometry.cpp:844-859
__device__ __forceinline__ bool ray_sphere(V3 o, V3 dir, float radius) {
	const V3 L = V3{0.0f - o.x, 0.0f - o.y, 0.0f - o.z};
	const float tca = dot(L, dir);
	const float d2 = dot(L, L) - tca * tca;
	if (d2 > radius * radius) return false;
	const float thc = sqrtf(radius * radius - d2);
	const float t = tca - thc;
	const float out = t >= 0 ? t : tca + thc;
	return out >= 0;
}

// (skin_point, evaluateSkin of model.cpp:103-109 over the palette: lmx_skin_eval.h)

__device__ __forceinline__ uint32_t load_index(const uint8_t* indices, const RayMeshRec& me, uint32_t i) {
	if (me.index_bytes == 2) return reinterpret_cast<const uint16_t*>(indices + me.index_at)[i];
	return reinterpret_cast<const uint32_t*>(indices + me.index_at)[i];
}

// Triangle `tri` of mesh `me` against the model-space ray. `pal` != nullptr: the candidate is skinned (a mesh without a skin still is not).
__device__ __forceinline__ bool test_mesh_triangle(const RaysDevice& d, const RayMeshRec& me, uint32_t tri, const float4* pal, uint32_t n_bones, V3 o, V3 dir, float* t) {
	V3 p[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t v = load_index(d.indices, me, 3 * tri + k); // (< n_verts: checked when the mesh was added)
		const float* q = d.positions + 3 * ((size_t)me.vert_at + v);
		p[k] = V3{q[0], q[1], q[2]};
		if (pal && me.skin_at != 0xffffffffu) p[k] = skin_point(pal, n_bones, d.skins[(size_t)me.skin_at + v], p[k]);
	}
	return ray_triangle(p[0], p[1], p[2], o, dir, t);
}

// the LOD-0 mesh (relative to the model's first) that holds triangle ordinal `ord`, walking on from `m`
__device__ __forceinline__ uint32_t mesh_of(const RayMeshRec* meshes, uint32_t n_meshes, uint32_t m, uint32_t ord) {
	while (m + 1 < n_meshes && ord >= meshes[m + 1].first_tri) ++m;
	return m;
}

__device__ __forceinline__ unsigned long long hit_key(float t, uint32_t index) {
	const uint32_t bits = t == 0 ? 0u : __float_as_uint(t); // -0 orders as +0
	return (unsigned long long)bits << 32 | index;
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_broad(RaysDevice d) {
	__shared__ LmxRay s_rays[RAY_BROAD_RAYS];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_rt = (d.n_rays + RAY_BROAD_RAYS - 1) / RAY_BROAD_RAYS;
	const uint32_t n_et = (d.n_inst + RAY_BLOCK - 1) / RAY_BLOCK;
	if (n_rt == 0) return;
	// pair p = et * n_rt + rt for p = blockIdx.x, + RAY_BROAD_GRID, ...: kept as (et, rt), stepped without a 64-bit division
	const uint32_t et_step = RAY_BROAD_GRID / n_rt, rt_step = RAY_BROAD_GRID % n_rt;
	uint32_t cur_et = 0xffffffffu;
	// the thread's entity
	bool ok = false;
	uint32_t e = 0, model = 0, palette_at = RAY_NO_PALETTE, n_bones = 0;
	RayTr tr = {};
	V3 inv_scale = {}, mn = {}, mx = {};
	float radius = 0, reach = 0;
	uint32_t rt = blockIdx.x % n_rt;
	for (uint32_t et = blockIdx.x / n_rt; et < n_et; et += et_step) {
		if (rt >= n_rt) { // (the carry of the step before)
			rt -= n_rt;
			if (++et >= n_et) break;
		}
		if (et != cur_et) {
			cur_et = et;
			e = et * RAY_BLOCK + threadIdx.x;
			ok = false;
			if (e < d.n_inst) {
				const int32_t m = d.inst_model[e];
				if ((d.inst_flags[e] & (INSTANCE_ENABLED | INSTANCE_VALID)) != 0 && m >= 0 && (uint32_t)m < d.n_models) {
					const RayModelRec& mo = d.models[m];
					if (mo.ready) {
						ok = true;
						model = (uint32_t)m;
						tr = load_ray_tr(d, e);
						inv_scale = V3{safe_inverse_scale(tr.scale.x), safe_inverse_scale(tr.scale.y), safe_inverse_scale(tr.scale.z)};
						radius = mo.radius;
						reach = radius * maximum3(tr.scale.x, tr.scale.y, tr.scale.z);
						mn = V3{mo.aabb_min[0], mo.aabb_min[1], mo.aabb_min[2]};
						const V3 size = sub(V3{mo.aabb_max[0], mo.aabb_max[1], mo.aabb_max[2]}, mn);
						mx = add(mn, size);
						palette_at = RAY_NO_PALETTE;
						n_bones = 0;
						if (mo.last_skinned && d.palette && e < d.n_skin_entities) { // `pose && !mesh.skin.empty() && pose->count <= 256` of the LAST mesh (model.cpp:147-150)
							const int32_t si = d.skin_of_entity[e];
							if (si >= 0 && (uint32_t)si < d.n_skin_inst && d.skin_inst[si].n_bones <= RAY_MAX_BONES) {
								palette_at = d.skin_inst[si].bone_offset;
								n_bones = d.skin_inst[si].n_bones;
							}
						}
					}
				}
			}
		}
		__syncthreads(); // (the previous tile's rays are no longer read)
		const uint32_t ray0 = rt * RAY_BROAD_RAYS;
		const uint32_t n_tile = d.n_rays - ray0 < RAY_BROAD_RAYS ? d.n_rays - ray0 : RAY_BROAD_RAYS;
		if (threadIdx.x < n_tile) s_rays[threadIdx.x] = d.rays[ray0 + threadIdx.x];
		__syncthreads();
		for (uint32_t r = 0; r < n_tile; ++r) { // (block-uniform: every lane takes every ballot)
			const LmxRay& ray = s_rays[r];
			bool pass = ok && (int32_t)e != ray.ignore;
			V3 o = {}, dir = {};
			if (pass) {
				const DV3 origin = DV3{ray.origin[0], ray.origin[1], ray.origin[2]};
				const double dist = length_d(sub(tr.pos, origin));
				if (dist - reach > (double)ray.t_max) pass = false;
				if (pass) {
					const DV3 rotated = rotate(conjugated(tr.rot), sub(origin, tr.pos)); // Transform::invTransform(DVec3), math.cpp:767-774
					o = to_v3(DV3{rotated.x * inv_scale.x, rotated.y * inv_scale.y, rotated.z * inv_scale.z});
					const V3 rv = rotate(conjugated(tr.rot), V3{ray.dir[0], ray.dir[1], ray.dir[2]}); // invTransformVector, math.cpp:789-797
					const V3 v = V3{rv.x * inv_scale.x, rv.y * inv_scale.y, rv.z * inv_scale.z};
					const float inv_len = 1 / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); // normalize, math.cpp:367-376
					dir = V3{v.x * inv_len, v.y * inv_len, v.z * inv_len};
					pass = ray_sphere(o, dir, radius) && ray_aabb(o, dir, mn, mx);
				}
			}
			// The append is written out, with lane 0 as the leader (every lane is here): lmx_wave.h's wave_append picks its leader from the
			// ballot, which this loop pays once per ray - the kernel's average over tools/ray_time.py's batches was 90.7-90.8 ms with it
			// against 90.1-90.3 ms (k_imray_broad below: 23.2 against 21.1-21.2 ms; k_pgray_broad: 99.4-99.7 against 98.7-98.9 us).
			const unsigned long long mask = __ballot(pass);
			if (mask == 0) continue; // (wave-uniform)
			unsigned long long base = 0; // (64 bits: rays x entities can pass 2^32, and the count is the size a larger reserve needs)
			if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long*>(d.state + RAYS_COUNTER), (unsigned long long)__popcll(mask));
			base = __shfl(base, 0);
			const unsigned long long slot = base + rank_in(mask);
			if (pass && slot < d.max_cand) {
				RayCandidate c;
				c.ray = ray0 + r; c.entity = e;
				c.o[0] = o.x; c.o[1] = o.y; c.o[2] = o.z;
				c.d[0] = dir.x; c.d[1] = dir.y; c.d[2] = dir.z;
				c.model = model; c.palette_at = palette_at; c.n_bones = n_bones; c.pad = 0;
				d.cand[slot] = c;
				d.cand_best[slot] = RAY_NONE;
			}
		}
		rt += rt_step; // (< 2 n_rt)
	}
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_narrow(RaysDevice d) {
	__shared__ float4 s_pal[RAY_MAX_BONES * 3];
	const uint32_t n_cand = candidates(d);
	const uint32_t part = blockIdx.x % RAY_NARROW_SPLIT;
	for (uint32_t c = blockIdx.x / RAY_NARROW_SPLIT; c < n_cand; c += RAY_NARROW_GRID / RAY_NARROW_SPLIT) {
		const RayCandidate cd = d.cand[c];
		const RayModelRec& mo = d.models[cd.model];
		const uint32_t n_tris = mo.n_tris;
		if ((uint64_t)part * RAY_CHUNK >= n_tris) continue; // (block-uniform)
		const bool skinned = cd.palette_at != RAY_NO_PALETTE;
		if (skinned) {
			__syncthreads(); // (the previous candidate's palette is no longer read)
			const float4* src = d.palette + (size_t)cd.palette_at * 3;
			for (uint32_t k = threadIdx.x; k < cd.n_bones * 3; k += RAY_BLOCK) s_pal[k] = src[k];
			__syncthreads();
		}
		const RayMeshRec* meshes = d.meshes + mo.first_mesh;
		const V3 o = V3{cd.o[0], cd.o[1], cd.o[2]}, dir = V3{cd.d[0], cd.d[1], cd.d[2]};
		unsigned long long best = RAY_NONE;
		uint32_t m = 0;
		for (uint64_t chunk = part; chunk * RAY_CHUNK < n_tris; chunk += RAY_NARROW_SPLIT) {
			const uint64_t first = chunk * RAY_CHUNK + (uint64_t)threadIdx.x * RAY_RUN;
			for (uint32_t k = 0; k < RAY_RUN; ++k) {
				if (first + k >= n_tris) break;
				const uint32_t ord = (uint32_t)(first + k);
				m = mesh_of(meshes, mo.n_meshes, m, ord);
				float t;
				if (test_mesh_triangle(d, meshes[m], ord - meshes[m].first_tri, skinned ? s_pal : nullptr, cd.n_bones, o, dir, &t)) {
					const unsigned long long key = hit_key(t, ord);
					if (key < best) best = key;
				}
			}
		}
		for (int off = 32; off > 0; off >>= 1) { // (every lane of the wave is here: the loops above hold no barrier)
			const unsigned long long other = __shfl_xor(best, off);
			if (other < best) best = other;
		}
		if ((threadIdx.x & 63u) == 0 && best != RAY_NONE) atomicMin(&d.cand_best[c], best);
	}
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_resolve(RaysDevice d) {
	const uint32_t n_cand = candidates(d);
	for (uint32_t c = blockIdx.x * RAY_BLOCK + threadIdx.x; c < n_cand; c += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const unsigned long long best = d.cand_best[c];
		if (best == RAY_NONE) continue;
		const RayCandidate cd = d.cand[c];
		const RayModelRec& mo = d.models[cd.model];
		const RayMeshRec* meshes = d.meshes + mo.first_mesh;
		const uint32_t ord = (uint32_t)best;
		const uint32_t m = mesh_of(meshes, mo.n_meshes, 0, ord);
		const V3 o = V3{cd.o[0], cd.o[1], cd.o[2]}, dir = V3{cd.d[0], cd.d[1], cd.d[2]};
		float t = __uint_as_float((uint32_t)(best >> 32));
		// the triangle's own t (the cell holds -0 as +0): the same loads and the same arithmetic give the same bits
		test_mesh_triangle(d, meshes[m], ord - meshes[m].first_tri, cd.palette_at != RAY_NO_PALETTE ? d.palette + (size_t)cd.palette_at * 3 : nullptr, cd.n_bones, o, dir, &t);
		// :2743-2745; hit.origin = DVec3(origin), model.cpp:220
		const V3 step = mul(dir, t);
		const V3 hit_model = to_v3(DV3{(double)o.x + step.x, (double)o.y + step.y, (double)o.z + step.z});
		const RayTr tr = load_ray_tr(d, cd.entity);
		const V3 rotated = rotate(tr.rot, V3{hit_model.x * tr.scale.x, hit_model.y * tr.scale.y, hit_model.z * tr.scale.z}); // Transform::transform(Vec3), math.cpp:765
		const DV3 hit_world = add(tr.pos, rotated);
		const LmxRay& ray = d.rays[cd.ray];
		const float new_t = (float)length_d(sub(DV3{ray.origin[0], ray.origin[1], ray.origin[2]}, hit_world));
		d.cand_t[c] = new_t;
		if (new_t < ray.t_max) atomicMin(&d.ray_best[cd.ray], hit_key(new_t, cd.entity)); // (a length: >= 0, or NaN and then not below t_max)
	}
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_write(RaysDevice d) {
	const uint32_t n_cand = candidates(d);
	const uint32_t gid = blockIdx.x * RAY_BLOCK + threadIdx.x;
	for (uint32_t r = gid; r < d.n_rays; r += RAY_RESOLVE_GRID * RAY_BLOCK) {
		if (d.ray_best[r] != RAY_NONE) continue; // (a candidate below writes it)
		LmxRayHit h;
		h.is_hit = 0; h.entity = 0; h.mesh = 0; h.triangle = 0; h.t = 0.0f; h.t_model = 0.0f;
		d.hits[r] = h;
	}
	for (uint32_t c = gid; c < n_cand; c += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const unsigned long long best = d.cand_best[c];
		if (best == RAY_NONE) continue;
		const RayCandidate cd = d.cand[c];
		const float new_t = d.cand_t[c];
		if (!(new_t < d.rays[cd.ray].t_max) || d.ray_best[cd.ray] != hit_key(new_t, cd.entity)) continue; // (one candidate per (ray, entity): one winner)
		const RayModelRec& mo = d.models[cd.model];
		const RayMeshRec* meshes = d.meshes + mo.first_mesh;
		const uint32_t ord = (uint32_t)best;
		const uint32_t m = mesh_of(meshes, mo.n_meshes, 0, ord);
		float t = __uint_as_float((uint32_t)(best >> 32));
		test_mesh_triangle(d, meshes[m], ord - meshes[m].first_tri, cd.palette_at != RAY_NO_PALETTE ? d.palette + (size_t)cd.palette_at * 3 : nullptr, cd.n_bones,
			V3{cd.o[0], cd.o[1], cd.o[2]}, V3{cd.d[0], cd.d[1], cd.d[2]}, &t);
		LmxRayHit h;
		h.is_hit = 1; h.entity = (int32_t)cd.entity; h.mesh = mo.mesh_base + m; h.triangle = ord - meshes[m].first_tri; h.t = new_t; h.t_model = t;
		d.hits[cd.ray] = h;
	}
	if (gid == 0) {
		const unsigned long long n = *reinterpret_cast<const unsigned long long*>(d.state + RAYS_COUNTER);
		d.state[RAYS_RAYS] = d.n_rays;
		d.state[RAYS_CANDIDATES] = n < 0xffffffffull ? (uint32_t)n : 0xffffffffu;
		d.state[RAYS_OVERFLOW] = (n > d.max_cand ? 1u : 0u) | d.state[RAYS_IM_OVERFLOW]; // (bit 1: the instanced-model stage ahead of this one overflowed; zero without one)
	}
}

// ---- instanced models ----

__global__ __launch_bounds__(RAY_BLOCK) void k_imray_broad(ImRaysDevice q) {
	__shared__ LmxRay s_rays[RAY_BROAD_RAYS];
	__shared__ V3 s_base[RAY_BROAD_RAYS];
	constexpr uint32_t SUB = IM_TILE / RAY_BLOCK; // 256-slot tiles of an IM_TILE tile
	static_assert(SUB * RAY_BLOCK == IM_TILE, "a 256-slot tile belongs to one model");
	const RaysDevice& d = q.r;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_rt = (d.n_rays + RAY_BROAD_RAYS - 1) / RAY_BROAD_RAYS;
	const uint32_t n_it = q.n_tiles * SUB;
	if (n_rt == 0) return;
	// pair p = it * n_rt + rt, stepped as in k_ray_broad
	const uint32_t it_step = RAY_IM_BROAD_GRID / n_rt, rt_step = RAY_IM_BROAD_GRID % n_rt;
	uint32_t cur_it = 0xffffffffu;
	// the tile's model (block-uniform) and the thread's instance
	bool live = false, ok = false;
	uint32_t slot = 0, model = 0, im = 0;
	int32_t entity = 0;
	DV3 origin = {};
	V3 pos = {};
	Q4 rot = {};
	float radius = 0, inv_scale = 0;
	uint32_t rt = blockIdx.x % n_rt;
	for (uint32_t it = blockIdx.x / n_rt; it < n_it; it += it_step) {
		if (rt >= n_rt) { // (the carry of the step before)
			rt -= n_rt;
			if (++it >= n_it) break;
		}
		if (it != cur_it) {
			cur_it = it;
			const uint32_t tile = it / SUB;
			im = q.tile_model[tile];
			live = ok = false;
			if (im < q.n_im_models) {
				const ImModelDev& mo = q.im_models[im];
				const RayImModelRec rm = q.im_ray_models[im];
				const uint32_t at = (tile - mo.first_tile) * IM_TILE + (it % SUB) * RAY_BLOCK; // the tile's first instance within the model
				live = at < mo.n && rm.ray_model >= 0 && (uint32_t)rm.ray_model < d.n_models && d.models[rm.ray_model].ready != 0; // `!im.model || !isReady()`, :2616
				if (live) {
					model = (uint32_t)rm.ray_model;
					entity = rm.entity;
					origin = DV3{mo.origin[0], mo.origin[1], mo.origin[2]};
					ok = at + threadIdx.x < mo.n; // (the slots behind are padding up to the next model)
					if (ok) {
						slot = mo.first + at + threadIdx.x;
						const float4 ps = q.pos_scale[slot], r4 = q.rot[slot];
						pos = V3{ps.x, ps.y, ps.z};
						radius = mo.radius * ps.w;                                                       // :2629
						rot = Q4{r4.x, r4.y, r4.z, sqrtf(1 - (r4.x * r4.x + r4.y * r4.y + r4.z * r4.z))}; // getInstanceQuat, :2619-2626
						inv_scale = 1 / ps.w;                                                            // Vec3::operator/(float), math.cpp:471-474
					}
				}
			}
		}
		if (!live) { // (block-uniform: a tile of padding, or a model that is not cast)
			rt += rt_step;
			continue;
		}
		__syncthreads(); // (the previous tile's rays are no longer read)
		const uint32_t ray0 = rt * RAY_BROAD_RAYS;
		const uint32_t n_tile = d.n_rays - ray0 < RAY_BROAD_RAYS ? d.n_rays - ray0 : RAY_BROAD_RAYS;
		if (threadIdx.x < n_tile) {
			const LmxRay ray = d.rays[ray0 + threadIdx.x];
			s_rays[threadIdx.x] = ray;
			s_base[threadIdx.x] = to_v3(sub(DV3{ray.origin[0], ray.origin[1], ray.origin[2]}, origin)); // Vec3(ray.origin - tr.pos), :2628
		}
		__syncthreads();
		for (uint32_t r = 0; r < n_tile; ++r) { // (block-uniform: every lane takes every ballot)
			const LmxRay& ray = s_rays[r];
			bool pass = ok && entity != ray.ignore; // the filter of :2603-2607 refuses every triangle of the model
			V3 o = {}, dir = {};
			if (pass) {
				const V3 rd = V3{ray.dir[0], ray.dir[1], ray.dir[2]};
				const V3 rel = sub(s_base[r], pos);
				pass = ray_sphere(rel, rd, radius);
				if (pass) {
					dir = rotate(conjugated(rot), rd); // (not normalised)
					o = rotate(conjugated(rot), V3{rel.x * inv_scale, rel.y * inv_scale, rel.z * inv_scale});
				}
			}
			const unsigned long long mask = __ballot(pass); // (written out, lane 0 leads: see k_ray_broad)
			if (mask == 0) continue; // (wave-uniform)
			unsigned long long base = 0;
			if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long*>(d.state + RAYS_COUNTER), (unsigned long long)__popcll(mask));
			base = __shfl(base, 0);
			const unsigned long long at = base + rank_in(mask);
			if (pass && at < d.max_cand) {
				RayCandidate c;
				c.ray = ray0 + r; c.entity = slot;
				c.o[0] = o.x; c.o[1] = o.y; c.o[2] = o.z;
				c.d[0] = dir.x; c.d[1] = dir.y; c.d[2] = dir.z;
				c.model = model; c.palette_at = RAY_NO_PALETTE; c.n_bones = 0; c.pad = im;
				d.cand[at] = c;
				d.cand_best[at] = RAY_NONE;
			}
		}
		rt += rt_step; // (< 2 n_rt)
	}
}

// the winning triangle of a candidate with a hit: its mesh (relative to LOD 0's first), its index there and its own t (the cell holds -0 as +0)
__device__ __forceinline__ float im_winner(const RaysDevice& d, const RayCandidate& cd, unsigned long long best, uint32_t* mesh, uint32_t* triangle) {
	const RayModelRec& mo = d.models[cd.model];
	const RayMeshRec* meshes = d.meshes + mo.first_mesh;
	const uint32_t ord = (uint32_t)best;
	const uint32_t m = mesh_of(meshes, mo.n_meshes, 0, ord);
	float t = __uint_as_float((uint32_t)(best >> 32));
	test_mesh_triangle(d, meshes[m], ord - meshes[m].first_tri, nullptr, 0, V3{cd.o[0], cd.o[1], cd.o[2]}, V3{cd.d[0], cd.d[1], cd.d[2]}, &t);
	*mesh = mo.mesh_base + m;
	*triangle = ord - meshes[m].first_tri;
	return t;
}

__global__ __launch_bounds__(RAY_BLOCK) void k_imray_resolve(ImRaysDevice q) {
	const RaysDevice& d = q.r;
	const uint32_t n_cand = candidates(d);
	for (uint32_t c = blockIdx.x * RAY_BLOCK + threadIdx.x; c < n_cand; c += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const unsigned long long best = d.cand_best[c];
		if (best == RAY_NONE) continue;
		const RayCandidate cd = d.cand[c];
		uint32_t mesh, triangle;
		const float t = im_winner(d, cd, best, &mesh, &triangle);
		const float scaled = t * q.pos_scale[cd.entity].w; // new_hit.t * id.scale, :2636
		d.cand_t[c] = scaled;
		if (scaled < d.rays[cd.ray].t_max) atomicMin(&q.im_best[cd.ray], ordered_key(scaled, cd.entity)); // (a NaN is below nothing)
	}
}

__global__ __launch_bounds__(RAY_BLOCK) void k_imray_write(ImRaysDevice q) {
	const RaysDevice& d = q.r;
	const uint32_t n_cand = candidates(d);
	const uint32_t gid = blockIdx.x * RAY_BLOCK + threadIdx.x;
	for (uint32_t r = gid; r < d.n_rays; r += RAY_RESOLVE_GRID * RAY_BLOCK) {
		if (q.im_best[r] != RAY_NONE) continue; // (a candidate below writes both)
		LmxRayImHit h;
		h.is_hit = 0; h.entity = 0; h.model = 0; h.subindex = 0; h.mesh = 0; h.triangle = 0; h.t = 0.0f; h.t_model = 0.0f;
		q.im_hits[r] = h;
		q.rays_eff[r] = d.rays[r];
	}
	for (uint32_t c = gid; c < n_cand; c += RAY_RESOLVE_GRID * RAY_BLOCK) {
		const unsigned long long best = d.cand_best[c];
		if (best == RAY_NONE) continue;
		const RayCandidate cd = d.cand[c];
		const float scaled = d.cand_t[c];
		LmxRay ray = d.rays[cd.ray];
		if (!(scaled < ray.t_max) || q.im_best[cd.ray] != ordered_key(scaled, cd.entity)) continue; // (one candidate per (ray, slot): one winner)
		LmxRayImHit h;
		h.t_model = im_winner(d, cd, best, &h.mesh, &h.triangle);
		h.is_hit = 1; h.entity = q.im_ray_models[cd.pad].entity; h.model = cd.pad; h.subindex = cd.entity - q.im_models[cd.pad].first; h.t = scaled;
		q.im_hits[cd.ray] = h;
		ray.t_max = scaled; // cur_dist = hit.t (:2719); `new_t < hit.t` (:2746)
		q.rays_eff[cd.ray] = ray;
	}
	if (gid == 0) {
		const unsigned long long n = *reinterpret_cast<const unsigned long long*>(d.state + RAYS_COUNTER);
		d.state[RAYS_RAYS] = d.n_rays;
		d.state[RAYS_CANDIDATES] = n < 0xffffffffull ? (uint32_t)n : 0xffffffffu;
		d.state[RAYS_OVERFLOW] = n > d.max_cand ? 1u : 0u;
		q.entity_state[RAYS_IM_OVERFLOW] = n > d.max_cand ? 2u : 0u;
	}
}

} // namespace

hipError_t launch_rays_broad(hipStream_t s, const RaysDevice& d) {
	hipLaunchKernelGGL(k_ray_broad, dim3(RAY_BROAD_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_rays_narrow(hipStream_t s, const RaysDevice& d) {
	hipLaunchKernelGGL(k_ray_narrow, dim3(RAY_NARROW_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_rays_resolve(hipStream_t s, const RaysDevice& d) {
	hipLaunchKernelGGL(k_ray_resolve, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_ray_write, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_imrays_broad(hipStream_t s, const ImRaysDevice& d) {
	hipLaunchKernelGGL(k_imray_broad, dim3(RAY_IM_BROAD_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_imrays_resolve(hipStream_t s, const ImRaysDevice& d) {
	hipLaunchKernelGGL(k_imray_resolve, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_imray_write, dim3(RAY_RESOLVE_GRID), dim3(RAY_BLOCK), 0, s, d);
	return hipGetLastError();
}

} // namespace lmx
