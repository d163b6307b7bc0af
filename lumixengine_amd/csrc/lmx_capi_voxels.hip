// lmx_capi_voxels.hip — the voxel entry points (include/lumix_mi355.h, "Voxels"): Voxels of renderer/voxels.cpp as an object beside the
// context. The host side validates, computes what the reference computes once per call (beginRaster's grid, voxelize's AABB in index
// order, the generator's state behind a computeAO) with the functions the kernels use (lmx_voxels.h), and launches voxel_kernels.hip.
#include "lmx_context.h"
#include "lmx_voxels.h"

#include <cfloat>
#include <cmath>

using namespace lmx;

struct LmxVoxels {
	LmxContext* ctx = nullptr;
	VoxelGrid g = {};
	uint32_t n_cells = 0;
	bool rastered = false; // beginRaster ran: the grid exists
	bool has_ao = false;   // computeAO ran on this grid
	bool has_rng = false;
	bool ao_lds = true;    // LMX_VOXELS_OPT_AO_LDS
	VoxelRng rng = {0, 0}; // the generator behind the last computeAO
	DevBuf<uint8_t> d_voxels, d_out_u8, d_inside;
	DevBuf<float> d_ao, d_ao_alt, d_tris, d_points, d_out_f;
};

namespace {

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// beginRaster's arithmetic with the refusals of the header; `why` names the first one
int grid_of(const float aabb_min[3], const float aabb_max[3], uint32_t max_res, VoxelGrid* g, const char** why) {
	*why = nullptr;
	if (!aabb_min || !aabb_max) *why = "null AABB";
	else if (max_res == 0) *why = "max_res is 0";
	else if (!finite3(aabb_min) || !finite3(aabb_max)) *why = "the AABB is not finite";
	if (*why) return LMX_ERR_INVALID_ARGUMENT;
	*g = voxel_grid(aabb_min, aabb_max, max_res);
	if (!(g->voxel_size > 0.0f) || !std::isfinite(g->voxel_size) || !finite3(g->mn) || !finite3(g->mx)) *why = "the AABB has no positive finite extent";
	else if (g->res[0] < 0 || g->res[1] < 0 || g->res[2] < 0) *why = "the AABB is inverted or its resolution leaves the i32 range";
	else if (voxel_cells(*g) > 0x7fffffffull || (uint64_t)(uint32_t)g->res[0] * (uint32_t)g->res[1] > 0x7fffffffull) *why = "the grid holds more than 2^31 - 1 cells";
	return *why ? LMX_ERR_INVALID_ARGUMENT : LMX_OK;
}

int check_mesh(LmxContext* ctx, const LmxVoxelsMesh& m) {
	if (m.index_count == 0) return LMX_OK;
	if (!m.positions || !m.indices) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: null positions / indices");
	if (m.stride_bytes < 12) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: a vertex stride of %u bytes holds no Vec3", m.stride_bytes);
	if (m.index_bytes != 2 && m.index_bytes != 4) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: indices of %u bytes (2 or 4)", m.index_bytes);
	if (m.index_count % 3 != 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: %u indices are no whole triangles", m.index_count);
	return LMX_OK;
}
uint32_t index_at(const LmxVoxelsMesh& m, uint32_t i) { // forEachTriangle (voxels.cpp:8-31)
	if (m.index_bytes == 2) { uint16_t v; memcpy(&v, (const uint8_t*)m.indices + 2 * (size_t)i, 2); return v; }
	uint32_t v; memcpy(&v, (const uint8_t*)m.indices + 4 * (size_t)i, 4); return v;
}
// the vertex an index refers to; false for an index past n_vertices or a position that is not finite
int vertex_at(LmxContext* ctx, const LmxVoxelsMesh& m, uint32_t i, float out[3]) {
	const uint32_t idx = index_at(m, i);
	if (idx >= m.n_vertices) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: index %u (at %u) past %u vertices", idx, i, m.n_vertices);
	memcpy(out, (const uint8_t*)m.positions + (size_t)idx * m.stride_bytes, 12);
	if (!finite3(out)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: vertex %u is not finite", idx);
	return LMX_OK;
}

int begin_raster(LmxVoxels* vox, const float aabb_min[3], const float aabb_max[3], uint32_t max_res) {
	LmxContext* ctx = vox->ctx;
	VoxelGrid g;
	const char* why;
	if (int rc = grid_of(aabb_min, aabb_max, max_res, &g, &why)) return fail(ctx, rc, "voxels: %s", why);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (a queued kernel may still read the buffer a reserve frees)
	const uint32_t n = (uint32_t)voxel_cells(g);
	LMX_HIP(ctx, vox->d_voxels.reserve(std::max<size_t>(n, 1)));
	if (n) LMX_HIP(ctx, hipMemsetAsync(vox->d_voxels.p, 0, n, ctx->stream));
	vox->g = g;
	vox->n_cells = n;
	vox->rastered = true;
	vox->has_ao = false; // (the reference keeps a stale m_ao of another size; nothing reads it before the next computeAO)
	return LMX_OK;
}

int raster_mesh(LmxVoxels* vox, const LmxVoxelsMesh& m) {
	LmxContext* ctx = vox->ctx;
	if (int rc = check_mesh(ctx, m)) return rc;
	const uint32_t n_tris = m.index_count / 3;
	if (!n_tris) return LMX_OK;
	std::vector<float> tris(9 * (size_t)n_tris);
	uint64_t most = 0; // the largest cell box of a triangle, cut to the grid
	for (uint32_t t = 0; t < n_tris; ++t) {
		float* p = tris.data() + 9 * (size_t)t;
		for (uint32_t k = 0; k < 3; ++k)
			if (int rc = vertex_at(ctx, m, 3 * t + k, p + 3 * k)) return rc;
		const VoxelSpan s = voxel_clip_box(vox->g, voxel_triangle_box(vox->g, V3{p[0], p[1], p[2]}, V3{p[3], p[4], p[5]}, V3{p[6], p[7], p[8]}));
		most = std::max(most, s.n);
	}
	const uint32_t split = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((most + VOXEL_RASTER_CELLS_PER_WAVE - 1) / VOXEL_RASTER_CELLS_PER_WAVE, 1), VOXEL_RASTER_MAX_SPLIT);
	if (int rc = upload_settled(ctx, vox->d_tris, tris.data(), tris.size())) return rc;
	LMX_HIP(ctx, launch_voxel_raster(ctx->stream, vox->g, vox->d_tris.p, n_tris, split, vox->d_voxels.p));
	return LMX_OK;
}

// points -> the three device arrays of a lookup; mode as k_voxel_sample takes it
int run_sample(LmxVoxels* vox, int mode, const float* packed_xyz, uint32_t n, float min_ao) {
	LmxContext* ctx = vox->ctx;
	if (int rc = upload_settled(ctx, vox->d_points, packed_xyz, 3 * (size_t)n)) return rc;
	// (the stream has drained: nothing reads the buffers a reserve frees)
	LMX_HIP(ctx, vox->d_out_u8.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, vox->d_out_f.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, vox->d_inside.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, launch_voxel_sample(ctx->stream, vox->g, mode, vox->d_voxels.p, vox->d_ao.p, vox->d_points.p, n, min_ao, vox->d_out_u8.p, vox->d_out_f.p, vox->d_inside.p));
	return LMX_OK;
}

} // namespace

extern "C" {

int lmx_voxels_grid(const float aabb_min[3], const float aabb_max[3], uint32_t max_res, LmxVoxelsInfo* out) {
	if (!out) return LMX_ERR_INVALID_ARGUMENT;
	VoxelGrid g;
	const char* why;
	if (int rc = grid_of(aabb_min, aabb_max, max_res, &g, &why)) return rc;
	for (int k = 0; k < 3; ++k) {
		out->aabb_min[k] = g.mn[k];
		out->aabb_max[k] = g.mx[k];
		out->resolution[k] = g.res[k];
	}
	out->voxel_size = g.voxel_size;
	return LMX_OK;
}

int lmx_voxels_rng_skip(uint32_t u, uint32_t v, uint64_t n, uint32_t* u_out, uint32_t* v_out) {
	if (!u_out || !v_out) return LMX_ERR_INVALID_ARGUMENT;
	const VoxelRng r = voxel_rng_skip(VoxelRng{u, v}, n);
	*u_out = r.u;
	*v_out = r.v;
	return LMX_OK;
}

int lmx_voxels_create(LmxContext* ctx, LmxVoxels** out) { return object_create(ctx, out, "voxels"); }

void lmx_voxels_destroy(LmxVoxels* vox) {
	if (vox) object_destroy(vox);
}

int lmx_voxels_set(LmxVoxels* dst, const LmxVoxels* src) {
	LMX_ENTER(dst);
	if (!src || src->ctx != ctx) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: the source is null or of another context");
	if (dst == src) return LMX_OK;
	if (!src->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: the source holds no grid");
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, dst->d_voxels.reserve(std::max<size_t>(src->n_cells, 1)));
	LMX_HIP(ctx, device_copy_on_stream(dst->d_voxels.p, (const uint8_t*)src->d_voxels.p, src->n_cells, ctx->stream));
	if (src->has_ao) {
		LMX_HIP(ctx, dst->d_ao.reserve(std::max<size_t>(src->n_cells, 1)));
		LMX_HIP(ctx, device_copy_on_stream(dst->d_ao.p, (const float*)src->d_ao.p, src->n_cells, ctx->stream));
	}
	dst->g = src->g;
	dst->n_cells = src->n_cells;
	dst->rastered = true;
	dst->has_ao = src->has_ao;
	return LMX_OK;
}

int lmx_voxels_begin_raster(LmxVoxels* vox, const float aabb_min[3], const float aabb_max[3], uint32_t max_res) {
	LMX_ENTER(vox);
	return begin_raster(vox, aabb_min, aabb_max, max_res);
}

int lmx_voxels_raster(LmxVoxels* vox, const void* positions, uint32_t stride_bytes, uint32_t n_vertices, const void* indices, uint32_t index_bytes, uint32_t index_count) {
	LMX_ENTER(vox);
	if (!vox->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: raster before begin_raster");
	const LmxVoxelsMesh m = {positions, stride_bytes, n_vertices, indices, index_bytes, index_count};
	return raster_mesh(vox, m);
}

int lmx_voxels_voxelize(LmxVoxels* vox, const LmxVoxelsMesh* meshes, uint32_t n_meshes, uint32_t max_res) {
	LMX_ENTER(vox);
	if (n_meshes && !meshes) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: null meshes");
	// the AABB over the vertices the indices reference, in index order (voxels.cpp:234-247): minimum(min, p) keeps `min` unless it is greater
	float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
	for (uint32_t k = 0; k < n_meshes; ++k) {
		if (int rc = check_mesh(ctx, meshes[k])) return rc;
		for (uint32_t i = 0; i < meshes[k].index_count; ++i) {
			float p[3];
			if (int rc = vertex_at(ctx, meshes[k], i, p)) return rc;
			for (int a = 0; a < 3; ++a) {
				mn[a] = vx_min(mn[a], p[a]);
				mx[a] = vx_max(mx[a], p[a]);
			}
		}
	}
	if (int rc = begin_raster(vox, mn, mx, max_res)) return rc;
	for (uint32_t k = 0; k < n_meshes; ++k)
		if (int rc = raster_mesh(vox, meshes[k])) return rc;
	return LMX_OK;
}

int lmx_voxels_compute_ao(LmxVoxels* vox, uint32_t ray_count, uint32_t seed_u, uint32_t seed_v) {
	LMX_ENTER(vox);
	if (!vox->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: compute_ao before a raster");
	if (ray_count == 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: ray_count is 0");
	if (seed_u == 0 || seed_v == 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: a generator half is 0 (RandomGenerator asserts both are not)");
	const uint64_t rays = (uint64_t)vox->n_cells * ray_count; // < 2^63: three draws each stay inside 64 bits
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, vox->d_ao.reserve(std::max<size_t>(vox->n_cells, 1)));
	const VoxelRng seed = VoxelRng{seed_u, seed_v};
	LMX_HIP(ctx, launch_voxel_ao(ctx->stream, vox->g, vox->d_voxels.p, ray_count, seed, vox->d_ao.p, vox->ao_lds));
	vox->rng = voxel_rng_skip(seed, 3 * rays);
	vox->has_rng = true;
	vox->has_ao = true;
	return LMX_OK;
}

int lmx_voxels_set_option(LmxVoxels* vox, int option, int value) {
	LMX_ENTER(vox);
	if (option != LMX_VOXELS_OPT_AO_LDS || (value != 0 && value != 1)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: option %d = %d", option, value);
	vox->ao_lds = value != 0;
	return LMX_OK;
}

int lmx_voxels_rng_state(LmxVoxels* vox, uint32_t* u, uint32_t* v) {
	LMX_ENTER(vox);
	if (!u || !v) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!vox->has_rng) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: no compute_ao has run");
	*u = vox->rng.u;
	*v = vox->rng.v;
	return LMX_OK;
}

int lmx_voxels_blur_ao(LmxVoxels* vox) {
	LMX_ENTER(vox);
	if (!vox->has_ao) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: blur_ao before compute_ao");
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, vox->d_ao_alt.reserve(std::max<size_t>(vox->n_cells, 1)));
	LMX_HIP(ctx, launch_voxel_blur(ctx->stream, vox->g, vox->d_ao.p, vox->d_ao_alt.p));
	vox->d_ao.swap(vox->d_ao_alt); // `m_ao = blurred.move()`
	return LMX_OK;
}

int lmx_voxels_sample(LmxVoxels* vox, const float* points_xyz, uint32_t n, uint8_t* out_u8, uint8_t* out_inside) {
	LMX_ENTER(vox);
	if (!vox->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: sample before a raster");
	if (!n) return LMX_OK;
	if (!points_xyz || !out_u8 || !out_inside) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: null points / outputs");
	if (int rc = run_sample(vox, VOXEL_SAMPLE_VOXEL, points_xyz, n, 0.f)) return rc;
	std::vector<uint8_t> value(n);
	LMX_HIP(ctx, read_back(value.data(), (const uint8_t*)vox->d_out_u8.p, n, ctx->stream));
	if (int rc = read_now(ctx, out_inside, (const uint8_t*)vox->d_inside.p, n)) return rc;
	for (uint32_t i = 0; i < n; ++i)
		if (out_inside[i]) out_u8[i] = value[i]; // (`*out` is written only where the point lies inside)
	return LMX_OK;
}

int lmx_voxels_sample_ao(LmxVoxels* vox, const float* points_xyz, uint32_t n, float* out_ao, uint8_t* out_inside) {
	LMX_ENTER(vox);
	if (!vox->has_ao) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: sample_ao before compute_ao");
	if (!n) return LMX_OK;
	if (!points_xyz || !out_ao || !out_inside) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: null points / outputs");
	if (int rc = run_sample(vox, VOXEL_SAMPLE_AO, points_xyz, n, 0.f)) return rc;
	std::vector<float> value(n);
	LMX_HIP(ctx, read_back(value.data(), (const float*)vox->d_out_f.p, n, ctx->stream));
	if (int rc = read_now(ctx, out_inside, (const uint8_t*)vox->d_inside.p, n)) return rc;
	for (uint32_t i = 0; i < n; ++i)
		if (out_inside[i]) out_ao[i] = value[i];
	return LMX_OK;
}

int lmx_voxels_bake_vertex_ao(LmxVoxels* vox, const void* positions, uint32_t stride_bytes, uint32_t n, float min_ao, uint8_t* out_u8) {
	LMX_ENTER(vox);
	if (!vox->has_ao) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: bake_vertex_ao before compute_ao");
	if (!n) return LMX_OK;
	if (!positions || !out_u8) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: null positions / output");
	if (stride_bytes < 12) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "voxels: a vertex stride of %u bytes holds no Vec3", stride_bytes);
	std::vector<float> packed(3 * (size_t)n);
	for (uint32_t i = 0; i < n; ++i) memcpy(packed.data() + 3 * (size_t)i, (const uint8_t*)positions + (size_t)i * stride_bytes, 12);
	if (int rc = run_sample(vox, VOXEL_SAMPLE_BAKE, packed.data(), n, min_ao)) return rc;
	std::vector<uint8_t> value(n), inside(n);
	LMX_HIP(ctx, read_back(value.data(), (const uint8_t*)vox->d_out_u8.p, n, ctx->stream));
	if (int rc = read_now(ctx, inside.data(), (const uint8_t*)vox->d_inside.p, n)) return rc;
	for (uint32_t i = 0; i < n; ++i)
		if (inside[i]) out_u8[i] = value[i]; // model_importer.cpp:1345: a vertex outside the grid keeps its byte
	return LMX_OK;
}

int lmx_voxels_info(LmxVoxels* vox, LmxVoxelsInfo* out) {
	LMX_ENTER(vox);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!vox->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: no grid");
	for (int k = 0; k < 3; ++k) {
		out->aabb_min[k] = vox->g.mn[k];
		out->aabb_max[k] = vox->g.mx[k];
		out->resolution[k] = vox->g.res[k];
	}
	out->voxel_size = vox->g.voxel_size;
	return LMX_OK;
}

int lmx_voxels_read(LmxVoxels* vox, uint8_t* out, uint32_t cap) {
	LMX_ENTER(vox);
	if (!vox->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: no grid");
	return read_out(ctx, out, cap, (const uint8_t*)vox->d_voxels.p, vox->n_cells, vox->n_cells, "cells", NullOut::Refused);
}

int lmx_voxels_read_ao(LmxVoxels* vox, float* out, uint32_t cap) {
	LMX_ENTER(vox);
	if (!vox->has_ao) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: no AO");
	return read_out(ctx, out, cap, (const float*)vox->d_ao.p, vox->n_cells, vox->n_cells, "cells of AO", NullOut::Refused);
}

int lmx_voxels_device_outputs(LmxVoxels* vox, LmxVoxelsDevice* out) {
	LMX_ENTER(vox);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!vox->rastered) return fail(ctx, LMX_ERR_NOT_BUILT, "voxels: no grid");
	out->d_voxels = vox->d_voxels.p;
	out->d_ao = vox->has_ao ? vox->d_ao.p : nullptr;
	out->n_cells = vox->n_cells;
	out->pad = 0;
	return LMX_OK;
}

} // extern "C"
