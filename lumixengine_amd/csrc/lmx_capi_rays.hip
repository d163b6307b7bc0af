// lmx_capi_rays.hip — castRay entry points (include/lumix_mi355.h, "ray casts" section): the geometry tables (LOD-0 meshes, models), the
// model instances by entity, the launch chain of ray_kernels.hip over a batch of rays and the read-backs. lmx_rays_cast enqueues and
// returns: the candidate count never reaches the host.
#include "lmx_context.h"
#include "lmx_im.h"

using namespace lmx;

namespace {

constexpr size_t GUARD_RECORDS = RAYS_GUARD_BYTES / sizeof(RayCandidate);
static_assert(GUARD_RECORDS * sizeof(RayCandidate) == RAYS_GUARD_BYTES, "whole records");

static_assert(sizeof(LmxRay) == 48 && sizeof(LmxRayHit) == 24 && sizeof(LmxRayModel) == 44, "ray records");
static_assert(sizeof(LmxRaysCounts) == 3 * sizeof(uint32_t), "read out of the state words");
static_assert(sizeof(LmxRayImHit) == 32 && sizeof(LmxRaysImCounts) == 3 * sizeof(uint32_t), "instanced-model records");

// the instanced-model stage's buffers, once there is both an attached object and a reserve
int rays_im_reserve(LmxContext* ctx) {
	RaysState& rs = ctx->rays;
	if (!rs.im || !rs.reserved) return LMX_OK;
	const size_t n = std::max<size_t>(rs.max_rays, 1);
	if (rs.d_im_best.cap >= n && rs.d_im_hits.cap >= n && rs.d_rays_eff.cap >= n && rs.d_im_state.p) return LMX_OK;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, rs.d_im_best.reserve(n));
	LMX_HIP(ctx, rs.d_im_hits.reserve(n));
	LMX_HIP(ctx, rs.d_rays_eff.reserve(n));
	LMX_HIP(ctx, rs.d_im_state.reserve(RAYS_STATE_WORDS));
	LMX_HIP(ctx, hipMemsetAsync(rs.d_im_state.p, 0, RAYS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	return LMX_OK;
}

// castRayInstancedModels over the attached object: fills q, enqueues the stage. The entity stage behind it casts q.rays_eff.
int rays_im_pass(LmxContext* ctx, const RaysDevice& d, ImRaysDevice& q) {
	RaysState& rs = ctx->rays;
	ImRayTables t;
	if (int rc = im_ray_tables(rs.im, &t)) return rc;
	if (rs.im_uploaded != t.n_models || rs.im_ray_models.size() != t.n_models) { // (models registered since the attach have no ray-table model)
		rs.im_ray_models.resize(t.n_models, RayImModelRec{-1, -1});
		if (int rc = upload_settled(ctx, rs.d_im_ray_models, rs.im_ray_models.data(), t.n_models)) return rc;
		rs.im_uploaded = t.n_models;
	}
	if (int rc = rays_im_reserve(ctx)) return rc;
	memset(&q, 0, sizeof(q));
	q.r = d;
	q.r.state = rs.d_im_state.p;
	q.r.hits = nullptr;
	q.im_models = t.models; q.n_im_models = t.n_models;
	q.tile_model = t.tile_model; q.n_tiles = t.n_tiles;
	q.pos_scale = t.pos_scale; q.rot = t.rot;
	q.im_ray_models = rs.d_im_ray_models.p;
	q.im_best = rs.d_im_best.p; q.im_hits = rs.d_im_hits.p; q.rays_eff = rs.d_rays_eff.p;
	q.entity_state = rs.d_state.p;
	LMX_HIP(ctx, hipMemsetAsync(rs.d_im_state.p, 0, RAYS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	if (d.n_rays) LMX_HIP(ctx, hipMemsetAsync(rs.d_im_best.p, 0xff, (size_t)d.n_rays * sizeof(unsigned long long), ctx->stream));
	LMX_HIP(ctx, launch_imrays_broad(ctx->stream, q));
	LMX_HIP(ctx, launch_rays_narrow(ctx->stream, q.r));
	LMX_HIP(ctx, launch_imrays_resolve(ctx->stream, q));
	return LMX_OK;
}

int rays_upload_meshes(LmxContext* ctx) {
	RaysState& rs = ctx->rays;
	if (!rs.meshes_dirty) return LMX_OK;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_meshes, rs.meshes, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_positions, rs.positions, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_skins, rs.skins, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_indices, rs.indices, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	rs.meshes_dirty = false;
	return LMX_OK;
}

int rays_pass(LmxContext* ctx, const LmxRay* d_rays, uint32_t n) {
	RaysState& rs = ctx->rays;
	if (!rs.have_models) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_set_models has not been called");
	if (!rs.have_instances) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_set_instances has not been called");
	if (!rs.reserved) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_reserve has not been called");
	if (n > rs.max_rays) return fail(ctx, LMX_ERR_CAPACITY, "%u rays: %u reserved", n, rs.max_rays);
	RaysDevice d;
	memset(&d, 0, sizeof(d));
	if (int rc = bind_entity_transforms(ctx, d)) return rc;
	if (int rc = rays_upload_meshes(ctx)) return rc;
	d.rays = d_rays; d.n_rays = n;
	d.inst_model = rs.d_inst_model.p; d.inst_flags = rs.d_inst_flags.p; d.n_inst = rs.n_inst;
	d.models = rs.d_models.p; d.n_models = rs.n_models;
	d.meshes = rs.d_meshes.p; d.positions = rs.d_positions.p; d.skins = rs.d_skins.p; d.indices = rs.d_indices.p;
	SkinState& sk = ctx->skin;
	if (ctx->poses.have_instances && sk.palette_valid && !sk.inst.empty()) { // "pose": a skin instance for the entity and a palette for the instance
		d.skin_of_entity = ctx->poses.d_skin_of_entity.p; d.n_skin_entities = ctx->poses.n_entities;
		d.skin_inst = sk.d_inst.p; d.n_skin_inst = (uint32_t)sk.inst.size();
		d.palette = sk.d_palette.p;
	}
	d.cand = rs.d_cand.p; d.max_cand = rs.max_cand;
	d.cand_best = rs.d_cand_best.p; d.cand_t = rs.d_cand_t.p; d.ray_best = rs.d_ray_best.p;
	d.hits = rs.d_hits.p; d.state = rs.d_state.p;
	rs.ran = rs.im_ran = rs.scene_ran = false;
	rs.n_rays = n;
	LMX_HIP(ctx, hipMemsetAsync(rs.d_state.p, 0, RAYS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	if (rs.im) { // the instanced models first; the entities see its hits as their rays' t_max. The entity stage's cursor is zero from the line above.
		ImRaysDevice q;
		if (int rc = rays_im_pass(ctx, d, q)) return rc;
		d.rays = q.rays_eff;
	}
	if (n) LMX_HIP(ctx, hipMemsetAsync(rs.d_ray_best.p, 0xff, (size_t)n * sizeof(unsigned long long), ctx->stream));
	LMX_HIP(ctx, launch_rays_broad(ctx->stream, d));
	LMX_HIP(ctx, launch_rays_narrow(ctx->stream, d));
	LMX_HIP(ctx, launch_rays_resolve(ctx->stream, d));
	if (rs.scene()) // procedural geometry, terrains and castRay's merge (:2761-2775) behind it
		if (int rc = rays_scene_pass(ctx, d, d_rays, rs.im ? rs.d_im_hits.p : nullptr)) return rc;
	rs.ran = true;
	rs.im_ran = rs.im != nullptr;
	rs.scene_ran = rs.scene();
	return LMX_OK;
}

} // namespace

extern "C" {

int lmx_rays_clear_meshes(LmxContext* ctx) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	rs.meshes.clear(); rs.positions.clear(); rs.skins.clear(); rs.indices.clear();
	rs.meshes_dirty = true;
	rs.have_models = false; // (their mesh ids are gone)
	rs.n_models = 0;
	return LMX_OK;
}

int lmx_rays_add_mesh(LmxContext* ctx, uint32_t n_verts, const float* positions_xyz, const LmxSkin* skin, const void* indices, uint32_t index_bytes, uint32_t index_count,
	uint32_t* out_mesh) {
	LMX_CHECK_CTX(ctx);
	if ((n_verts && !positions_xyz) || (index_count && !indices)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null input array");
	if (index_bytes != 2 && index_bytes != 4) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "index width %u: 2 or 4 bytes", index_bytes);
	if (index_count % 3) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%u indices: not a triangle list", index_count);
	for (uint32_t i = 0; i < index_count; ++i) {
		const uint32_t v = index_bytes == 2 ? ((const uint16_t*)indices)[i] : ((const uint32_t*)indices)[i];
		if (v >= n_verts) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "index %u = %u: the mesh has %u vertices", i, v, n_verts);
	}
	RaysState& rs = ctx->rays;
	if (rs.positions.size() / 3 + n_verts > 0xfffffff0ull || rs.indices.size() + (uint64_t)index_count * index_bytes > 0xfffffff0ull)
		return fail(ctx, LMX_ERR_CAPACITY, "the mesh tables' offsets are 32 bits");
	RayMeshRec me;
	memset(&me, 0, sizeof(me));
	me.n_tris = index_count / 3;
	me.index_at = (uint32_t)rs.indices.size();
	me.index_bytes = index_bytes;
	me.vert_at = (uint32_t)(rs.positions.size() / 3);
	me.n_verts = n_verts;
	me.skin_at = skin ? (uint32_t)rs.skins.size() : 0xffffffffu;
	rs.positions.insert(rs.positions.end(), positions_xyz, positions_xyz + (size_t)n_verts * 3);
	if (skin) rs.skins.insert(rs.skins.end(), skin, skin + n_verts);
	rs.indices.insert(rs.indices.end(), (const uint8_t*)indices, (const uint8_t*)indices + (size_t)index_count * index_bytes);
	rs.indices.resize((rs.indices.size() + 3) & ~(size_t)3); // (the next mesh's 32-bit indices stay aligned)
	rs.meshes.push_back(me);
	rs.meshes_dirty = true;
	if (out_mesh) *out_mesh = (uint32_t)rs.meshes.size() - 1;
	return LMX_OK;
}

int lmx_rays_set_models(LmxContext* ctx, uint32_t n_models, const LmxRayModel* models) {
	LMX_CHECK_CTX(ctx);
	if (n_models && !models) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null model table");
	RaysState& rs = ctx->rays;
	std::vector<RayModelRec> recs(n_models);
	for (uint32_t m = 0; m < n_models; ++m) { // every model is checked before the shared mesh records change
		const LmxRayModel& in = models[m];
		if ((uint64_t)in.first_mesh + in.mesh_count > rs.meshes.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "model %u: meshes [%u, %u + %u) of %zu", m, in.first_mesh, in.first_mesh, in.mesh_count, rs.meshes.size());
		uint64_t tris = 0;
		for (uint32_t k = 0; k < in.mesh_count; ++k) tris += rs.meshes[in.first_mesh + k].n_tris;
		if (tris > 0xfffffff0ull) return fail(ctx, LMX_ERR_CAPACITY, "model %u: %llu triangles, the ordinal is 32 bits", m, (unsigned long long)tris);
	}
	for (uint32_t m = 0; m < n_models; ++m) {
		const LmxRayModel& in = models[m];
		RayModelRec& r = recs[m];
		memset(&r, 0, sizeof(r));
		for (int k = 0; k < 3; ++k) { r.aabb_min[k] = in.aabb_min[k]; r.aabb_max[k] = in.aabb_max[k]; }
		r.radius = in.origin_radius;
		r.ready = in.ready ? 1u : 0u;
		r.first_mesh = in.first_mesh; r.n_meshes = in.mesh_count; r.mesh_base = in.lod0_from;
		uint32_t tris = 0;
		for (uint32_t k = 0; k < in.mesh_count; ++k) { // a mesh's ordinals start where the model's meshes before it end
			RayMeshRec& me = rs.meshes[in.first_mesh + k];
			if (me.first_tri != tris) rs.meshes_dirty = true;
			me.first_tri = tris;
			tris += me.n_tris;
		}
		r.n_tris = tris;
		r.last_skinned = in.mesh_count && rs.meshes[in.first_mesh + in.mesh_count - 1].skin_at != 0xffffffffu ? 1u : 0u;
	}
	if (int rc = upload_settled(ctx, rs.d_models, recs.data(), recs.size())) return rc;
	rs.n_models = n_models;
	rs.have_models = true;
	return LMX_OK;
}

int lmx_rays_set_instances(LmxContext* ctx, uint32_t n_entities, const int32_t* model, const uint8_t* flags) {
	LMX_CHECK_CTX(ctx);
	if (n_entities && (!model || !flags)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null instance table");
	if (n_entities > (1u << 31)) return fail(ctx, LMX_ERR_CAPACITY, "%u entities: at most 2^31", n_entities);
	RaysState& rs = ctx->rays;
	if (!rs.have_models) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_set_models has not been called");
	for (uint32_t e = 0; e < n_entities; ++e)
		if (model[e] >= 0 && (uint32_t)model[e] >= rs.n_models) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %u: model %d of %u", e, model[e], rs.n_models);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_inst_model, model, n_entities, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_inst_flags, flags, n_entities, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	rs.n_inst = n_entities;
	rs.have_instances = true;
	return LMX_OK;
}

int lmx_rays_reserve(LmxContext* ctx, uint32_t max_rays, uint32_t max_candidates) {
	LMX_CHECK_CTX(ctx);
	if (max_rays > (1u << 30) || max_candidates > (1u << 30)) return fail(ctx, LMX_ERR_CAPACITY, "%u rays / %u candidates: at most 2^30", max_rays, max_candidates);
	RaysState& rs = ctx->rays;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, rs.d_rays.reserve(std::max<size_t>(max_rays, 1)));
	LMX_HIP(ctx, rs.d_hits.reserve(std::max<size_t>(max_rays, 1)));
	LMX_HIP(ctx, rs.d_ray_best.reserve(std::max<size_t>(max_rays, 1)));
	LMX_HIP(ctx, rs.d_cand.reserve((size_t)max_candidates + GUARD_RECORDS));
	LMX_HIP(ctx, rs.d_cand_best.reserve(std::max<size_t>(max_candidates, 1)));
	LMX_HIP(ctx, rs.d_cand_t.reserve(std::max<size_t>(max_candidates, 1)));
	LMX_HIP(ctx, rs.d_state.reserve(RAYS_STATE_WORDS));
	LMX_HIP(ctx, fill_guard(rs.d_cand.p + max_candidates, GUARD_RECORDS, ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(rs.d_state.p, 0, RAYS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	rs.max_rays = max_rays;
	rs.max_cand = max_candidates;
	rs.reserved = true;
	rs.ran = rs.im_ran = rs.scene_ran = false;
	if (int rc = rays_im_reserve(ctx)) return rc;
	return rays_scene_reserve(ctx);
}

int lmx_rays_cast(LmxContext* ctx, const LmxRay* rays, uint32_t n) {
	LMX_CHECK_CTX(ctx);
	if (n && !rays) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null rays");
	RaysState& rs = ctx->rays;
	if (rs.reserved && n <= rs.max_rays && n) { // (the errors come from the pass)
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (a cast before this one may still read the rays)
		LMX_HIP(ctx, upload_on_stream(rs.d_rays.p, rays, n, ctx->stream));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's array has been read)
	}
	return rays_pass(ctx, rs.d_rays.p, n);
}

int lmx_rays_cast_device(LmxContext* ctx, const LmxRay* d_rays, uint32_t n) {
	LMX_CHECK_CTX(ctx);
	if (n && !d_rays) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null rays");
	return rays_pass(ctx, d_rays, n);
}

int lmx_rays_counts(LmxContext* ctx, LmxRaysCounts* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!ctx->rays.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_cast has not run");
	uint32_t c[3];
	if (int rc = read_now(ctx, c, ctx->rays.d_state.p, 3)) return rc;
	out->rays = c[RAYS_RAYS]; out->candidates = c[RAYS_CANDIDATES]; out->overflow = c[RAYS_OVERFLOW];
	return LMX_OK;
}

int lmx_rays_read_hits(LmxContext* ctx, LmxRayHit* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_cast has not run");
	return read_out(ctx, out, cap, (const LmxRayHit*)rs.d_hits.p, rs.n_rays, rs.n_rays, "hits");
}

int lmx_rays_read_candidates(LmxContext* ctx, void* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.reserved) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_reserve has not been called");
	return read_out(ctx, (RayCandidate*)out, cap, (const RayCandidate*)rs.d_cand.p, 0, (size_t)rs.max_cand + GUARD_RECORDS, "candidates"); // (the buffer from its start: any capacity)
}

int lmx_rays_device_outputs(LmxContext* ctx, const LmxRayHit** d_hits, const uint32_t** d_counts) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.reserved) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_reserve has not been called");
	if (d_hits) *d_hits = rs.d_hits.p;
	if (d_counts) *d_counts = rs.d_state.p;
	return LMX_OK;
}

int lmx_rays_set_instanced_models(LmxContext* ctx, LmxInstancedModels* im, uint32_t n_models, const int32_t* ray_model, const int32_t* entity) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!im) {
		rs.im = nullptr;
		rs.im_ran = false;
		return LMX_OK;
	}
	if (im_context(im) != ctx) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the instanced models belong to another context");
	if (n_models > im_model_count(im)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%u models: the object has %u", n_models, im_model_count(im));
	if (n_models && (!ray_model || !entity)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null model table");
	for (uint32_t m = 0; m < n_models; ++m)
		if (ray_model[m] >= 0 && (!rs.have_models || (uint32_t)ray_model[m] >= rs.n_models))
			return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instanced model %u: ray model %d of %u", m, ray_model[m], rs.have_models ? rs.n_models : 0u);
	rs.im_ray_models.resize(n_models);
	for (uint32_t m = 0; m < n_models; ++m) rs.im_ray_models[m] = RayImModelRec{ray_model[m] < 0 ? -1 : ray_model[m], entity[m]};
	rs.im_uploaded = ~(size_t)0;
	rs.im = im;
	rs.im_ran = false;
	return rays_im_reserve(ctx);
}

int lmx_rays_im_counts(LmxContext* ctx, LmxRaysImCounts* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	RaysState& rs = ctx->rays;
	if (!rs.ran || !rs.im_ran) return fail(ctx, LMX_ERR_NOT_BUILT, "no cast with instanced models attached has run");
	uint32_t c[3];
	if (int rc = read_now(ctx, c, rs.d_im_state.p, 3)) return rc;
	out->rays = c[RAYS_RAYS]; out->candidates = c[RAYS_CANDIDATES]; out->overflow = c[RAYS_OVERFLOW];
	return LMX_OK;
}

int lmx_rays_read_im_hits(LmxContext* ctx, LmxRayImHit* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.ran || !rs.im_ran) return fail(ctx, LMX_ERR_NOT_BUILT, "no cast with instanced models attached has run");
	return read_out(ctx, out, cap, (const LmxRayImHit*)rs.d_im_hits.p, rs.n_rays, rs.n_rays, "hits");
}

int lmx_rays_device_im_outputs(LmxContext* ctx, const LmxRayImHit** d_hits, const uint32_t** d_counts) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.reserved || !rs.im) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_reserve / lmx_rays_set_instanced_models has not been called");
	if (d_hits) *d_hits = rs.d_im_hits.p;
	if (d_counts) *d_counts = rs.d_im_state.p;
	return LMX_OK;
}

} // extern "C"
