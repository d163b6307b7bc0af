// lmx_capi_rays_scene.hip — procedural geometry and terrains in the cast (include/lumix_mi355.h, "ray casts" section): the two tables, the
// launch chain of ray_scene_kernels.hip behind the entity stage of lmx_capi_rays.hip and the read-backs. Nothing here waits for a cast.
#include "lmx_context.h"

using namespace lmx;

namespace {

static_assert(sizeof(LmxRayProcGeom) == 64 && sizeof(LmxRayTerrain) == 40, "table records");
static_assert(sizeof(LmxRayPgHit) == 20 && sizeof(LmxRayTerrainHit) == 28 && sizeof(LmxRaySceneHit) == 24, "hit records");
static_assert(sizeof(LmxRaysSceneCounts) == 3 * sizeof(uint32_t), "read out of the state words");

constexpr uint64_t MAX_TERRAIN_HITS = 1ull << 31; // rays x terrains records of a batch

int not_run(LmxContext* ctx) { return fail(ctx, LMX_ERR_NOT_BUILT, "no cast with procedural geometries or terrains set has run"); }

} // namespace

namespace lmx {

int rays_scene_reserve(LmxContext* ctx) {
	RaysState& rs = ctx->rays;
	if (!rs.reserved || !rs.scene()) return LMX_OK;
	const size_t n = std::max<size_t>(rs.max_rays, 1);
	const uint64_t pairs = (uint64_t)rs.max_rays * rs.n_terrains;
	if (pairs > MAX_TERRAIN_HITS) return fail(ctx, LMX_ERR_CAPACITY, "%u rays x %u terrains: at most 2^31 hit records", rs.max_rays, rs.n_terrains);
	const size_t n_th = std::max<size_t>((size_t)pairs, 1);
	if (rs.d_pg_best.cap >= n && rs.d_pg_hits.cap >= n && rs.d_scene_hits.cap >= n && rs.d_terrain_hits.cap >= n_th && rs.d_scene_state.p) return LMX_OK;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, rs.d_pg_best.reserve(n));
	LMX_HIP(ctx, rs.d_pg_hits.reserve(n));
	LMX_HIP(ctx, rs.d_scene_hits.reserve(n));
	LMX_HIP(ctx, rs.d_terrain_hits.reserve(n_th));
	LMX_HIP(ctx, rs.d_scene_state.reserve(RAYS_STATE_WORDS));
	LMX_HIP(ctx, hipMemsetAsync(rs.d_scene_state.p, 0, RAYS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	return LMX_OK;
}

int rays_scene_pass(LmxContext* ctx, const RaysDevice& d, const LmxRay* rays, const LmxRayImHit* im_hits) {
	RaysState& rs = ctx->rays;
	if (int rc = rays_scene_reserve(ctx)) return rc;
	SceneRaysDevice q;
	memset(&q, 0, sizeof(q));
	q.r = d;
	q.r.rays = rays;
	q.r.inst_model = nullptr; q.r.inst_flags = nullptr; q.r.n_inst = 0;
	q.r.models = rs.d_pg_models.p; q.r.n_models = rs.n_pg;
	q.r.meshes = rs.d_pg_meshes.p; q.r.positions = rs.d_pg_positions.p; q.r.indices = rs.d_pg_indices.p;
	q.r.skins = nullptr; q.r.skin_of_entity = nullptr; q.r.n_skin_entities = 0; q.r.skin_inst = nullptr; q.r.n_skin_inst = 0; q.r.palette = nullptr;
	q.r.ray_best = nullptr; q.r.hits = nullptr;
	q.r.state = rs.d_scene_state.p;
	q.pg = rs.d_pg.p; q.n_pg = rs.n_pg;
	q.pg_best = rs.d_pg_best.p; q.pg_hits = rs.d_pg_hits.p;
	q.terrains = rs.d_terrains.p; q.n_terrains = rs.n_terrains; q.texels = rs.d_texels.p;
	q.terrain_hits = rs.d_terrain_hits.p;
	q.hits = d.hits; q.im_hits = im_hits;
	q.scene_hits = rs.d_scene_hits.p;
	q.entity_state = d.state;
	const uint32_t n = d.n_rays;
	LMX_HIP(ctx, hipMemsetAsync(rs.d_scene_state.p, 0, RAYS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	if (rs.n_pg) {
		if (n) LMX_HIP(ctx, hipMemsetAsync(rs.d_pg_best.p, 0xff, (size_t)n * sizeof(unsigned long long), ctx->stream));
		LMX_HIP(ctx, launch_pgrays_broad(ctx->stream, q));
		LMX_HIP(ctx, launch_rays_narrow(ctx->stream, q.r));
		LMX_HIP(ctx, launch_pgrays_resolve(ctx->stream, q));
	} else if (n) {
		LMX_HIP(ctx, hipMemsetAsync(rs.d_pg_hits.p, 0, (size_t)n * sizeof(LmxRayPgHit), ctx->stream)); // (no geometry: no hit)
	}
	if (rs.n_terrains) LMX_HIP(ctx, launch_terrain_rays(ctx->stream, q));
	LMX_HIP(ctx, launch_scene_write(ctx->stream, q));
	return LMX_OK;
}

} // namespace lmx

extern "C" {

int lmx_rays_set_procedural_geometries(LmxContext* ctx, uint32_t n, const LmxRayProcGeom* geometries) {
	LMX_CHECK_CTX(ctx);
	if (n && !geometries) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null geometry table");
	RaysState& rs = ctx->rays;
	std::vector<RayPgRec> pg(n);
	std::vector<RayModelRec> models(n);
	std::vector<RayMeshRec> meshes(n);
	std::vector<float> positions;
	std::vector<uint8_t> indices;
	for (uint32_t g = 0; g < n; ++g) {
		const LmxRayProcGeom& in = geometries[g];
		if (in.index_bytes != 0 && in.index_bytes != 2 && in.index_bytes != 4) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "geometry %u: index width %u: 0, 2 or 4 bytes", g, in.index_bytes);
		const bool has_vertices = in.vertex_bytes != 0; // `pg.vertex_data.empty()`, :2655
		if (has_vertices && in.stride < 12) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "geometry %u: stride %u: a position takes 12 bytes", g, in.stride);
		if (has_vertices && !in.vertex_data) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "geometry %u: null vertex data", g);
		const bool castable = has_vertices && in.triangles != 0;
		const bool indexed = in.index_bytes != 0 && in.index_count != 0; // `pg.index_data.size() != 0`, :2671
		if (castable && indexed && !in.index_data) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "geometry %u: null index data", g);
		const uint32_t n_verts = castable ? in.vertex_bytes / in.stride : 0;
		const uint32_t n_tris = castable ? (indexed ? in.index_count : n_verts) / 3 : 0; // :2672, the integer divisions included
		pg[g] = RayPgRec{in.entity, castable ? 1u : 0u};
		RayModelRec& mo = models[g];
		memset(&mo, 0, sizeof(mo));
		for (int k = 0; k < 3; ++k) { mo.aabb_min[k] = in.aabb_min[k]; mo.aabb_max[k] = in.aabb_max[k]; }
		mo.ready = castable ? 1u : 0u;
		mo.first_mesh = g; mo.n_meshes = 1; mo.n_tris = n_tris;
		RayMeshRec& me = meshes[g];
		memset(&me, 0, sizeof(me));
		me.n_tris = n_tris;
		me.index_at = (uint32_t)indices.size();
		me.index_bytes = indexed && in.index_bytes == 2 ? 2 : 4;
		me.vert_at = (uint32_t)(positions.size() / 3);
		me.n_verts = n_verts;
		me.skin_at = 0xffffffffu;
		if (!castable) continue;
		if (positions.size() / 3 + n_verts > 0xfffffff0ull || indices.size() + (uint64_t)n_tris * 12 > 0xfffffff0ull)
			return fail(ctx, LMX_ERR_CAPACITY, "the geometry tables' offsets are 32 bits");
		for (uint32_t v = 0; v < n_verts; ++v) { // the memcpy of :2697-2699: the first 12 bytes at v * stride
			float p[3];
			memcpy(p, (const uint8_t*)in.vertex_data + (size_t)v * in.stride, sizeof(p));
			positions.insert(positions.end(), p, p + 3);
		}
		if (indexed) {
			for (uint32_t i = 0; i < 3 * n_tris; ++i) { // (the trailing indices are never read)
				uint32_t v;
				if (in.index_bytes == 2) { uint16_t w; memcpy(&w, (const uint8_t*)in.index_data + (size_t)i * 2, 2); v = w; }
				else memcpy(&v, (const uint8_t*)in.index_data + (size_t)i * 4, 4);
				if (v >= n_verts) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "geometry %u: index %u = %u: it has %u vertices", g, i, v, n_verts);
			}
			const uint8_t* src = (const uint8_t*)in.index_data;
			indices.insert(indices.end(), src, src + (size_t)3 * n_tris * in.index_bytes);
		} else { // tindices = {i, i + 1, i + 2}, :2692-2694
			for (uint32_t i = 0; i < 3 * n_tris; ++i) {
				const uint8_t* src = (const uint8_t*)&i;
				indices.insert(indices.end(), src, src + 4);
			}
		}
		indices.resize((indices.size() + 3) & ~(size_t)3); // (the next geometry's 32-bit indices stay aligned)
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_pg, pg, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_pg_models, models, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_pg_meshes, meshes, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_pg_positions, positions, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_pg_indices, indices, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	rs.n_pg = n;
	rs.scene_ran = false;
	return rays_scene_reserve(ctx);
}

int lmx_rays_set_terrains(LmxContext* ctx, uint32_t n, const LmxRayTerrain* terrains) {
	LMX_CHECK_CTX(ctx);
	if (n && !terrains) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null terrain table");
	if (n > RAY_MAX_TERRAINS) return fail(ctx, LMX_ERR_CAPACITY, "%u terrains: at most %u", n, RAY_MAX_TERRAINS);
	RaysState& rs = ctx->rays;
	if (rs.reserved && (uint64_t)rs.max_rays * n > MAX_TERRAIN_HITS) return fail(ctx, LMX_ERR_CAPACITY, "%u rays x %u terrains: at most 2^31 hit records", rs.max_rays, n);
	std::vector<RayTerrainRec> recs(n);
	uint64_t bytes = 0;
	for (uint32_t k = 0; k < n; ++k) {
		const LmxRayTerrain& in = terrains[k];
		if (in.format != LMX_RAY_TERRAIN_R16 && in.format != LMX_RAY_TERRAIN_RGBA8) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u: format %u", k, in.format);
		if (in.ready && (!in.texels || in.width == 0 || in.height == 0)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u: ready without a %u x %u heightmap", k, in.width, in.height);
		if (in.ready && (uint64_t)in.width * in.height > (1ull << 30)) return fail(ctx, LMX_ERR_CAPACITY, "terrain %u: %u x %u texels: at most 2^30", k, in.width, in.height);
		RayTerrainRec& r = recs[k];
		memset(&r, 0, sizeof(r));
		r.entity = in.entity; r.width = in.width; r.height = in.height; r.format = in.format;
		for (int c = 0; c < 3; ++c) r.scale[c] = in.scale[c];
		r.ready = in.ready ? 1u : 0u;
		r.texel_at = bytes;
		if (r.ready) bytes += ((uint64_t)in.width * in.height * (in.format == LMX_RAY_TERRAIN_R16 ? 2 : 4) + 3) & ~3ull;
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, rs.d_texels.reserve(std::max<size_t>((size_t)bytes, 1)));
	for (uint32_t k = 0; k < n; ++k) // the heightmaps go up as they are: 2 or 4 bytes per texel
		if (recs[k].ready)
			LMX_HIP(ctx, upload_on_stream(rs.d_texels.p + recs[k].texel_at, (const uint8_t*)terrains[k].texels, (size_t)terrains[k].width * terrains[k].height * (terrains[k].format == LMX_RAY_TERRAIN_R16 ? 2 : 4), ctx->stream));
	LMX_HIP(ctx, upload_on_stream(rs.d_terrains, recs, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	rs.n_terrains = n;
	rs.scene_ran = false;
	return rays_scene_reserve(ctx);
}

int lmx_rays_read_pg_hits(LmxContext* ctx, LmxRayPgHit* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.ran || !rs.scene_ran) return not_run(ctx);
	return read_out(ctx, out, cap, (const LmxRayPgHit*)rs.d_pg_hits.p, rs.n_rays, rs.n_rays, "hits");
}

int lmx_rays_read_terrain_hits(LmxContext* ctx, LmxRayTerrainHit* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.ran || !rs.scene_ran) return not_run(ctx);
	const size_t need = (size_t)rs.n_rays * rs.n_terrains;
	return read_out(ctx, out, cap, (const LmxRayTerrainHit*)rs.d_terrain_hits.p, need, need, "hits (rays x terrains)");
}

int lmx_rays_read_scene_hits(LmxContext* ctx, LmxRaySceneHit* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.ran || !rs.scene_ran) return not_run(ctx);
	return read_out(ctx, out, cap, (const LmxRaySceneHit*)rs.d_scene_hits.p, rs.n_rays, rs.n_rays, "hits");
}

int lmx_rays_scene_counts(LmxContext* ctx, LmxRaysSceneCounts* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	RaysState& rs = ctx->rays;
	if (!rs.ran || !rs.scene_ran) return not_run(ctx);
	uint32_t c[3];
	if (int rc = read_now(ctx, c, rs.d_scene_state.p, 3)) return rc;
	out->rays = c[RAYS_RAYS]; out->candidates = c[RAYS_CANDIDATES]; out->overflow = c[RAYS_OVERFLOW];
	return LMX_OK;
}

int lmx_rays_device_scene_outputs(LmxContext* ctx, const LmxRaySceneHit** d_hits, const uint32_t** d_counts) {
	LMX_CHECK_CTX(ctx);
	RaysState& rs = ctx->rays;
	if (!rs.reserved || !rs.scene()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_rays_reserve / lmx_rays_set_procedural_geometries / lmx_rays_set_terrains has not been called");
	if (d_hits) *d_hits = rs.d_scene_hits.p;
	if (d_counts) *d_counts = rs.d_scene_state.p;
	return LMX_OK;
}

} // extern "C"
