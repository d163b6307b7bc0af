// lmx_capi_clusters.hip — fillClusters entry points (include/lumix_mi355.h, "clustered lights and probes" section): the point-light and
// shadow-atlas tables by entity, the enabled probes in output order, the launch chain of cluster_kernels.hip over the LOCAL_LIGHT list
// of a cull result (or a caller's list) and the read-backs. lmx_clusters_run enqueues and returns: the list's length never reaches the host.
#include "lmx_context.h"

using namespace lmx;

namespace {

constexpr size_t GUARD_RECORDS = CLUSTERS_GUARD_BYTES / 64, GUARD_WORDS = CLUSTERS_GUARD_BYTES / 4;

static_assert(sizeof(LmxPointLight) == 32 && sizeof(LmxEnvProbe) == 136 && sizeof(LmxReflProbe) == 20, "table records");
static_assert(sizeof(ClusterEnvRec) == 208 && sizeof(ClusterReflRec) == 48, "ClusterEnvProbe / ClusterReflProbe (pipeline.cpp:3349-3366)");
static_assert(sizeof(LmxClusterPlanes) == 16 + sizeof(ClusterPlanesArg), "the planes go to the kernel as they are");
static_assert(sizeof(LmxClustersCounts) == 5 * sizeof(uint32_t), "read out of the state words");

// Ascending order of a volume product under `<`, as a total order: -0 == +0, NaN behind everything.
uint32_t order_key(float v) {
	if (v != v) return 0xffffffffu;
	if (v == 0.0f) v = 0.0f;
	uint32_t b;
	memcpy(&b, &v, 4);
	return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

// The enabled probes of one kind in output order: ascending volume (pipeline.cpp:3512-3516, :3534-3538), ties in module order.
template <typename P, typename F> std::vector<uint32_t> probe_order(const P* probes, uint32_t n, F volume) {
	std::vector<uint32_t> idx;
	for (uint32_t i = 0; i < n; ++i)
		if (probes[i].flags & LMX_PROBE_ENABLED) idx.push_back(i);
	std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return order_key(volume(probes[a])) < order_key(volume(probes[b])); });
	return idx;
}

float length3(const float v[3]) { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); } // core/math.cpp:392

int clusters_ready(LmxContext* ctx) {
	ClustersState& cl = ctx->clusters;
	if (!cl.have_lights) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_clusters_set_lights has not been called");
	if (!cl.reserved) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_clusters_reserve has not been called");
	return LMX_OK;
}

// The pass over `list_cap` entries at most of `d_list`, its length on the device.
int clusters_pass(LmxContext* ctx, const LmxClusterView* cv, const int32_t* d_list, const uint32_t* d_count, size_t list_cap) {
	ClustersState& cl = ctx->clusters;
	LmxClusterPlanes planes;
	if (lmx_clusters_planes(&cv->frustum, cv->viewport_w, cv->viewport_h, &planes) != LMX_OK)
		return fail(ctx, LMX_ERR_CAPACITY, "viewport %u x %u: more than %d x %d clusters", cv->viewport_w, cv->viewport_h, LMX_CLUSTER_MAX_XY, LMX_CLUSTER_MAX_XY);
	ClustersDevice d;
	memset(&d, 0, sizeof(d));
	if (int rc = bind_entity_transforms(ctx, d)) return rc;
	list_cap = std::min<size_t>(list_cap, 1u << 30);
	if (int rc = Grow{ctx}(cl.d_ranges, std::max<size_t>(list_cap, 1))) return rc; // (a pass of the previous view may still read the old ranges)
	d.list = d_list; d.list_count = d_count; d.list_cap = (uint32_t)list_cap;
	d.light_tab = cl.d_light_tab.p; d.n_light_tab = cl.n_light_tab;
	if (cl.have_atlas) { d.atlas = cl.d_atlas.p; d.n_atlas = cl.n_atlas; }
	d.env_entity = cl.d_env_entity.p; d.env_radius = cl.d_env_radius.p; d.env_tmpl = cl.d_env_tmpl.p; d.n_env = cl.n_env;
	d.refl_entity = cl.d_refl_entity.p; d.refl_radius = cl.d_refl_radius.p; d.refl_tmpl = cl.d_refl_tmpl.p; d.n_refl = cl.n_refl;
	for (int k = 0; k < 3; ++k) d.cam[k] = cv->camera_pos[k];
	d.size_x = planes.size[0]; d.size_y = planes.size[1]; d.size_z = planes.size[2];
	d.n_clusters = d.size_x * d.size_y * d.size_z;
	d.max_lights = cl.max_lights; d.map_capacity = cl.map_capacity;
	d.ranges = cl.d_ranges.p; d.probe_ranges = cl.d_probe_ranges.p; d.totals = cl.d_totals.p; d.offsets = cl.d_offsets.p;
	d.lights = cl.d_lights.p; d.light_entities = cl.d_light_entities.p; d.clusters = cl.d_clusters.p; d.map = cl.d_map.p;
	d.env_out = cl.d_env_out.p; d.refl_out = cl.d_refl_out.p; d.state = cl.d_state.p;
	ClusterPlanesArg pa;
	memcpy(pa.planes, planes.xplanes, sizeof(pa.planes));
	cl.ran = false;
	for (int k = 0; k < 3; ++k) cl.size[k] = planes.size[k];
	LMX_HIP(ctx, launch_cluster_records(ctx->stream, d, pa));
	LMX_HIP(ctx, launch_cluster_bins(ctx->stream, d));
	cl.ran = true;
	return LMX_OK;
}

int host_counts(LmxContext* ctx, uint32_t c[5]) {
	if (!ctx->clusters.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_clusters_run has not run");
	return read_now(ctx, c, ctx->clusters.d_state.p, 5);
}

} // namespace

extern "C" {

int lmx_clusters_set_lights(LmxContext* ctx, uint32_t n_entities, const LmxPointLight* lights) {
	LMX_CHECK_CTX(ctx);
	if (n_entities && !lights) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null light table");
	ClustersState& cl = ctx->clusters;
	if (int rc = upload_settled(ctx, cl.d_light_tab, lights, n_entities)) return rc;
	cl.n_light_tab = n_entities;
	cl.have_lights = true;
	return LMX_OK;
}

int lmx_clusters_set_atlas(LmxContext* ctx, uint32_t n_entities, const uint32_t* atlas_idx) {
	LMX_CHECK_CTX(ctx);
	ClustersState& cl = ctx->clusters;
	cl.have_atlas = false;
	cl.n_atlas = 0;
	if (!atlas_idx) return LMX_OK;
	if (int rc = upload_settled(ctx, cl.d_atlas, atlas_idx, n_entities)) return rc;
	cl.n_atlas = n_entities;
	cl.have_atlas = true;
	return LMX_OK;
}

int lmx_clusters_set_probes(LmxContext* ctx, uint32_t n_env, const LmxEnvProbe* env, const int32_t* env_entities, uint32_t n_refl, const LmxReflProbe* refl,
	const int32_t* refl_entities) {
	LMX_CHECK_CTX(ctx);
	if (n_env > LMX_CLUSTER_MAX_PROBES || n_refl > LMX_CLUSTER_MAX_PROBES)
		return fail(ctx, LMX_ERR_CAPACITY, "%u environment / %u reflection probes: at most %d of a kind", n_env, n_refl, LMX_CLUSTER_MAX_PROBES);
	if ((n_env && (!env || !env_entities)) || (n_refl && (!refl || !refl_entities))) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null probe table");
	ClustersState& cl = ctx->clusters;
	const std::vector<uint32_t> eo = probe_order(env, n_env, [](const LmxEnvProbe& p) { return p.outer_range[0] * p.outer_range[1] * p.outer_range[2]; });
	const std::vector<uint32_t> ro = probe_order(refl, n_refl, [](const LmxReflProbe& p) { return p.half_extents[0] * p.half_extents[1] * p.half_extents[2]; });
	std::vector<int32_t> e_ent(eo.size()), r_ent(ro.size());
	std::vector<float> e_rad(eo.size()), r_rad(ro.size());
	std::vector<ClusterEnvRec> e_rec(eo.size());
	std::vector<ClusterReflRec> r_rec(ro.size());
	for (size_t k = 0; k < eo.size(); ++k) { // ClusterEnvProbe of :3524-3531 with pos / rot left to the run; the pads are zero
		const LmxEnvProbe& p = env[eo[k]];
		e_ent[k] = env_entities[eo[k]];
		e_rad[k] = length3(p.outer_range);
		memset(&e_rec[k], 0, sizeof(ClusterEnvRec));
		e_rec[k].v[2] = make_float4(p.inner_range[0], p.inner_range[1], p.inner_range[2], 0.0f);
		e_rec[k].v[3] = make_float4(p.outer_range[0], p.outer_range[1], p.outer_range[2], 0.0f);
		for (int i = 0; i < 9; ++i) e_rec[k].v[4 + i] = make_float4(p.sh_coefs[i][0], p.sh_coefs[i][1], p.sh_coefs[i][2], 0.0f);
	}
	for (size_t k = 0; k < ro.size(); ++k) { // ClusterReflProbe of :3505-3509
		const LmxReflProbe& p = refl[ro[k]];
		r_ent[k] = refl_entities[ro[k]];
		r_rad[k] = length3(p.half_extents);
		memset(&r_rec[k], 0, sizeof(ClusterReflRec));
		memcpy(&r_rec[k].v[0].w, &p.texture_id, 4); // layer
		r_rec[k].v[2] = make_float4(p.half_extents[0], p.half_extents[1], p.half_extents[2], 0.0f);
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_on_stream(cl.d_env_entity, e_ent, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(cl.d_env_radius, e_rad, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(cl.d_env_tmpl, e_rec, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(cl.d_refl_entity, r_ent, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(cl.d_refl_radius, r_rad, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(cl.d_refl_tmpl, r_rec, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	cl.n_env = (uint32_t)eo.size();
	cl.n_refl = (uint32_t)ro.size();
	return LMX_OK;
}

int lmx_clusters_reserve(LmxContext* ctx, uint32_t max_lights, uint32_t map_capacity) {
	LMX_CHECK_CTX(ctx);
	if (max_lights > (1u << 30)) return fail(ctx, LMX_ERR_CAPACITY, "%u lights: at most 2^30", max_lights);
	ClustersState& cl = ctx->clusters;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, cl.d_lights.reserve(((size_t)max_lights + GUARD_RECORDS) * 4));
	LMX_HIP(ctx, cl.d_light_entities.reserve((size_t)max_lights + GUARD_WORDS));
	LMX_HIP(ctx, cl.d_map.reserve((size_t)map_capacity + GUARD_WORDS));
	LMX_HIP(ctx, cl.d_clusters.reserve(CLUSTER_MAX_CLUSTERS));
	LMX_HIP(ctx, cl.d_totals.reserve(CLUSTER_MAX_CLUSTERS));
	LMX_HIP(ctx, cl.d_offsets.reserve(CLUSTER_MAX_CLUSTERS));
	LMX_HIP(ctx, cl.d_probe_ranges.reserve(2 * LMX_CLUSTER_MAX_PROBES));
	LMX_HIP(ctx, cl.d_env_out.reserve(LMX_CLUSTER_MAX_PROBES));
	LMX_HIP(ctx, cl.d_refl_out.reserve(LMX_CLUSTER_MAX_PROBES));
	LMX_HIP(ctx, cl.d_state.reserve(CLUSTERS_STATE_WORDS));
	LMX_HIP(ctx, fill_guard(cl.d_lights.p + (size_t)max_lights * 4, GUARD_RECORDS * 4, ctx->stream));
	LMX_HIP(ctx, fill_guard(cl.d_light_entities.p + max_lights, GUARD_WORDS, ctx->stream));
	LMX_HIP(ctx, fill_guard(cl.d_map.p + map_capacity, GUARD_WORDS, ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(cl.d_state.p, 0, CLUSTERS_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	cl.max_lights = max_lights;
	cl.map_capacity = map_capacity;
	cl.reserved = true;
	cl.ran = false;
	return LMX_OK;
}

int lmx_clusters_run(LmxContext* ctx, uint32_t view, uint32_t frustum, const LmxClusterView* cv) {
	LMX_CHECK_CTX(ctx);
	if (!cv) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null view state");
	if (view >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view");
	if (int rc = clusters_ready(ctx)) return rc;
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u out of range", frustum);
	if (v.culled_type != LMX_TYPE_ALL && v.culled_type != LMX_TYPE_LOCAL_LIGHT)
		return fail(ctx, LMX_ERR_NOT_BUILT, "the cull in view %u covered type %u only, not LOCAL_LIGHT", view, v.culled_type);
	if (int rc = cull_view_consolidate(ctx, v)) return rc; // one contiguous list per type: two small launches, once per cull result
	return clusters_pass(ctx, cv, v.cons_ptr() + (size_t)frustum * v.out_stride + v.out_start[LMX_TYPE_LOCAL_LIGHT],
		v.totals_ptr() + frustum * MAX_TYPES + LMX_TYPE_LOCAL_LIGHT, v.out_cap[LMX_TYPE_LOCAL_LIGHT]);
}

int lmx_clusters_run_list(LmxContext* ctx, const LmxClusterView* cv, const int32_t* entities, uint32_t n) {
	LMX_CHECK_CTX(ctx);
	if (!cv) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null view state");
	if (n && !entities) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null list");
	if (n > (1u << 30)) return fail(ctx, LMX_ERR_CAPACITY, "%u listed lights: at most 2^30", n);
	if (int rc = clusters_ready(ctx)) return rc;
	ClustersState& cl = ctx->clusters;
	if (int rc = upload_list(ctx, cl.d_list, entities, n, cl.d_state.p + CLUSTERS_LIST_N, cl.list_n)) return rc;
	return clusters_pass(ctx, cv, cl.d_list.p, cl.d_state.p + CLUSTERS_LIST_N, n);
}

int lmx_clusters_counts(LmxContext* ctx, LmxClustersCounts* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	uint32_t c[5];
	if (int rc = host_counts(ctx, c)) return rc;
	out->lights = c[CLUSTERS_LIGHTS]; out->env_probes = c[CLUSTERS_ENV]; out->refl_probes = c[CLUSTERS_REFL]; out->map_entries = c[CLUSTERS_MAP];
	out->overflow = c[CLUSTERS_OVERFLOW];
	return LMX_OK;
}

int lmx_clusters_read_lights(LmxContext* ctx, void* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[5];
	if (int rc = host_counts(ctx, c)) return rc;
	ClustersState& cl = ctx->clusters;
	struct Rec { float4 v[4]; };
	return read_out(ctx, (Rec*)out, cap, (const Rec*)cl.d_lights.p, std::min(c[CLUSTERS_LIGHTS], cl.max_lights), (size_t)cl.max_lights + GUARD_RECORDS, "light records");
}

int lmx_clusters_read_light_entities(LmxContext* ctx, int32_t* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[5];
	if (int rc = host_counts(ctx, c)) return rc;
	ClustersState& cl = ctx->clusters;
	return read_out(ctx, out, cap, (const int32_t*)cl.d_light_entities.p, std::min(c[CLUSTERS_LIGHTS], cl.max_lights), (size_t)cl.max_lights + GUARD_WORDS, "light entities");
}

int lmx_clusters_read_clusters(LmxContext* ctx, void* out, uint32_t cap, uint32_t* size) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[5];
	if (int rc = host_counts(ctx, c)) return rc;
	ClustersState& cl = ctx->clusters;
	if (size) memcpy(size, cl.size, sizeof(cl.size));
	const size_t n = (size_t)cl.size[0] * cl.size[1] * cl.size[2];
	return read_out(ctx, (uint4*)out, cap, (const uint4*)cl.d_clusters.p, n, n, "clusters");
}

int lmx_clusters_read_map(LmxContext* ctx, int32_t* out, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[5];
	if (int rc = host_counts(ctx, c)) return rc;
	ClustersState& cl = ctx->clusters;
	return read_out(ctx, out, cap, (const int32_t*)cl.d_map.p, std::min(c[CLUSTERS_MAP], cl.map_capacity), (size_t)cl.map_capacity + GUARD_WORDS, "map entries");
}

int lmx_clusters_read_probes(LmxContext* ctx, void* env, uint32_t env_cap, void* refl, uint32_t refl_cap) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[5];
	if (int rc = host_counts(ctx, c)) return rc;
	ClustersState& cl = ctx->clusters;
	if (env)
		if (int rc = read_out(ctx, (ClusterEnvRec*)env, env_cap, (const ClusterEnvRec*)cl.d_env_out.p, c[CLUSTERS_ENV], c[CLUSTERS_ENV], "environment probes")) return rc;
	if (refl)
		if (int rc = read_out(ctx, (ClusterReflRec*)refl, refl_cap, (const ClusterReflRec*)cl.d_refl_out.p, c[CLUSTERS_REFL], c[CLUSTERS_REFL], "reflection probes")) return rc;
	return LMX_OK;
}

int lmx_clusters_device_outputs(LmxContext* ctx, LmxClustersDevice* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	ClustersState& cl = ctx->clusters;
	if (!cl.reserved) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_clusters_reserve has not been called");
	memset(out, 0, sizeof(*out));
	out->d_lights = cl.d_lights.p; out->d_light_entities = cl.d_light_entities.p; out->d_clusters = cl.d_clusters.p; out->d_map = cl.d_map.p;
	out->d_env_probes = cl.d_env_out.p; out->d_refl_probes = cl.d_refl_out.p; out->d_counts = cl.d_state.p;
	memcpy(out->size, cl.size, sizeof(cl.size));
	return LMX_OK;
}

} // extern "C"
