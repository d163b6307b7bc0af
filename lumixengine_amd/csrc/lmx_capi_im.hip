// lmx_capi_im.hip — instanced-model entry points (include/lumix_mi355.h, "Instanced models"): the model table, the device grid build of
// RenderModuleImpl::initInstancedModelGPUData and encodeInstancedModels for every model of a view (im_kernels.hip).
#include "lmx_context.h"
#include "lmx_im.h"

#include <cmath>

using namespace lmx;

struct LmxInstancedModels {
	LmxContext* ctx = nullptr;
	struct Model {
		float lod_dist[4] = {0, 0, 0, 0};
		LmxLodIndices lod_idx[5] = {};
		float radius = 0;
		std::vector<uint32_t> indices;
		uint32_t n = 0;
		double origin[3] = {0, 0, 0};
	};
	std::vector<Model> models;
	std::vector<ImModelDev> table;  // host copy of d_models (first / tiles / indirect offsets derived from `models`)
	std::vector<uint32_t> tile_model, indices;
	uint32_t n_tiles = 0, n_indirect = 0;
	size_t n_slots = 0, total_instances = 0;
	bool dirty = true;
	DevBuf<ImModelDev> d_models;
	DevBuf<ImGridDev> d_grids;
	DevBuf<uint32_t> d_tile_model, d_indices;
	DevBuf<float4> d_pos_scale, d_rot;
	DevBuf<float> d_lod;
	DevBuf<LmxImInstance> d_stage;
	DevBuf<uint64_t> d_masks;
	DevBuf<uint4> d_tile_counts;
	DevBuf<uint32_t> d_model_tot; // [2][n_models][4] bin totals of a run (k_im_count adds, k_im_emit clears the other half); zero where allocated
	uint32_t tot_parity = 0;
	struct Slot {
		DevBuf<LmxImInstance> records;
		DevBuf<LmxImIndirect> indirect;
		DevBuf<ImCountsDev> counts;
		bool valid = false;
		uint32_t n_models = 0, n_indirect = 0;
	} slots[LMX_MAX_VIEWS];
	ImArrays arrays() { return ImArrays{d_pos_scale.p, d_rot.p, d_lod.p}; }
};

namespace {

uint32_t tiles_of(uint32_t n) { return n ? (n + IM_TILE - 1) / IM_TILE : 1u; }
size_t span_of(uint32_t n) { return (size_t)((n + IM_TILE - 1) / IM_TILE) * IM_TILE; }

// Model table, tile list and indirect offsets from the host state; uploads them (the stream is idle: set_* calls synchronize first).
int im_upload_tables(LmxInstancedModels* im) {
	LmxContext* ctx = im->ctx;
	if (!im->dirty) return LMX_OK;
	const uint32_t nm = (uint32_t)im->models.size();
	im->table.assign(nm, ImModelDev{});
	im->tile_model.clear();
	im->indices.clear();
	size_t first = 0;
	for (uint32_t m = 0; m < nm; ++m) {
		const LmxInstancedModels::Model& src = im->models[m];
		ImModelDev& d = im->table[m];
		for (int k = 0; k < 4; ++k) d.lod_dist[k] = src.lod_dist[k];
		d.lod_idx[0] = src.lod_idx[0].to; // encodeInstancedModels: running maximum of the LODs' `to`
		for (int k = 1; k < 4; ++k) d.lod_idx[k] = std::max(d.lod_idx[k - 1], src.lod_idx[k].to);
		float dist = 0; // getDrawDistance (pipeline.cpp:2494-2503)
		for (int k = 0; k < 4; ++k)
			if (src.lod_idx[k].to != -1) dist = src.lod_dist[k];
		d.draw_distance = sqrtf(dist);
		d.radius = src.radius;
		d.first = (uint32_t)first;
		d.n = src.n;
		d.first_tile = (uint32_t)im->tile_model.size();
		d.n_tiles = tiles_of(src.n);
		for (uint32_t t = 0; t < d.n_tiles; ++t) im->tile_model.push_back(m);
		d.indirect_offset = (uint32_t)im->indices.size();
		d.mesh_count = (uint32_t)src.indices.size();
		im->indices.insert(im->indices.end(), src.indices.begin(), src.indices.end());
		for (int k = 0; k < 3; ++k) d.origin[k] = src.origin[k];
		first += span_of(src.n);
	}
	im->n_tiles = (uint32_t)im->tile_model.size();
	im->n_indirect = (uint32_t)im->indices.size();
	LMX_HIP(ctx, im->d_models.reserve(std::max<size_t>(nm, 1)));
	LMX_HIP(ctx, im->d_tile_model.reserve(std::max<size_t>(im->n_tiles, 1)));
	LMX_HIP(ctx, im->d_indices.reserve(std::max<size_t>(im->n_indirect, 1)));
	LMX_HIP(ctx, im->d_tile_counts.reserve(std::max<size_t>(im->n_tiles, 1)));
	if (im->d_model_tot.cap < 8 * (size_t)std::max<uint32_t>(nm, 1)) {
		LMX_HIP(ctx, im->d_model_tot.reserve(8 * (size_t)std::max<uint32_t>(nm, 1)));
		LMX_HIP(ctx, hipMemset(im->d_model_tot.p, 0, im->d_model_tot.cap * sizeof(uint32_t)));
	}
	LMX_HIP(ctx, upload_blocking(im->d_models.p, im->table));
	LMX_HIP(ctx, upload_blocking(im->d_tile_model.p, im->tile_model));
	LMX_HIP(ctx, upload_blocking(im->d_indices.p, im->indices));
	im->dirty = false;
	return LMX_OK;
}

// The instance arrays hold every model's span (a multiple of IM_TILE) back to back. A model whose span changes moves the ones behind it:
// the arrays are laid out again and the other models' instances (their LOD state included) are copied over on the device.
int im_relayout(LmxInstancedModels* im, uint32_t model, uint32_t new_n) {
	LmxContext* ctx = im->ctx;
	const uint32_t nm = (uint32_t)im->models.size();
	size_t total = 0, new_total = 0;
	std::vector<size_t> old_first(nm), new_first(nm);
	for (uint32_t m = 0; m < nm; ++m) {
		old_first[m] = total;
		new_first[m] = new_total;
		total += span_of(im->models[m].n);
		new_total += span_of(m == model ? new_n : im->models[m].n);
	}
	if (span_of(im->models[model].n) == span_of(new_n) && im->d_pos_scale.cap >= std::max<size_t>(total, 64)) return LMX_OK;
	DevBuf<float4> ps, rot;
	DevBuf<float> lod;
	DevBuf<uint64_t> masks;
	const size_t cap = std::max<size_t>(new_total, 64);
	LMX_HIP(ctx, ps.reserve(cap));
	LMX_HIP(ctx, rot.reserve(cap));
	LMX_HIP(ctx, lod.reserve(cap));
	LMX_HIP(ctx, masks.reserve(cap / 64 + 1));
	for (uint32_t m = 0; m < nm; ++m) {
		const uint32_t n = im->models[m].n;
		if (m == model || !n) continue;
		LMX_HIP(ctx, device_copy_blocking(ps.p + new_first[m], im->d_pos_scale.p + old_first[m], n));
		LMX_HIP(ctx, device_copy_blocking(rot.p + new_first[m], im->d_rot.p + old_first[m], n));
		LMX_HIP(ctx, device_copy_blocking(lod.p + new_first[m], im->d_lod.p + old_first[m], n));
	}
	im->d_pos_scale.swap(ps);
	im->d_rot.swap(rot);
	im->d_lod.swap(lod);
	im->d_masks.swap(masks);
	im->n_slots = new_total;
	return LMX_OK;
}

int im_check_slot(LmxInstancedModels* im, uint32_t view_slot) {
	if (view_slot >= LMX_MAX_VIEWS) return fail(im->ctx, LMX_ERR_INVALID_ARGUMENT, "view slot %u out of range (LMX_MAX_VIEWS = %d)", view_slot, LMX_MAX_VIEWS);
	if (!im->slots[view_slot].valid) return fail(im->ctx, LMX_ERR_NOT_BUILT, "view slot %u holds no instanced-model run", view_slot);
	return LMX_OK;
}

void invalidate_slots(LmxInstancedModels* im) {
	for (auto& s : im->slots) s.valid = false;
}

} // namespace

namespace lmx {

LmxContext* im_context(const LmxInstancedModels* im) { return im->ctx; }
uint32_t im_model_count(const LmxInstancedModels* im) { return (uint32_t)im->models.size(); }

int im_ray_tables(LmxInstancedModels* im, ImRayTables* out) {
	LmxContext* ctx = im->ctx;
	if (im->dirty) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (int rc = im_upload_tables(im)) return rc;
	}
	out->models = im->d_models.p; out->n_models = (uint32_t)im->models.size();
	out->tile_model = im->d_tile_model.p; out->n_tiles = im->n_tiles;
	out->pos_scale = im->d_pos_scale.p; out->rot = im->d_rot.p;
	return LMX_OK;
}

} // namespace lmx

extern "C" {

int lmx_im_create(LmxContext* ctx, LmxInstancedModels** out) { return object_create(ctx, out, "instanced models"); }

void lmx_im_destroy(LmxInstancedModels* im) {
	if (!im) return;
	if (im->ctx->rays.im == im) im->ctx->rays.im = nullptr; // (the ray casts no longer see it)
	object_destroy(im);
}

int lmx_im_set_model(LmxInstancedModels* im, uint32_t model, const float lod_distances[4], const LmxLodIndices lod_indices[5], float origin_radius,
	uint32_t mesh_count, const uint32_t* indices_count) {
	LMX_ENTER(im);
	if (!lod_distances || !lod_indices || (mesh_count && !indices_count)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null model array");
	if (model > im->models.size() || model >= LMX_IM_MAX_MODELS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "model %u: ids are dense (%zu registered)", model, im->models.size());
	if (mesh_count > LMX_IM_MAX_MESHES) return fail(ctx, LMX_ERR_CAPACITY, "%u meshes: encodeInstancedModels takes fewer than 32", mesh_count);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (model == im->models.size()) { // a new model: the grid table grows (keeping the others' grids) and its grid is that of no instance
		if (im->d_grids.cap < model + 1) {
			DevBuf<ImGridDev> grids;
			LMX_HIP(ctx, grids.reserve(model + 1));
			LMX_HIP(ctx, device_copy_blocking(grids.p, im->d_grids.p, model));
			im->d_grids.swap(grids);
		}
		LMX_HIP(ctx, launch_im_grid_build(ctx->stream, nullptr, 0, im->arrays(), 0, im->d_grids.p + model));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		im->models.emplace_back();
	}
	LmxInstancedModels::Model& md = im->models[model];
	for (int k = 0; k < 4; ++k) md.lod_dist[k] = lod_distances[k];
	for (int k = 0; k < 5; ++k) md.lod_idx[k] = lod_indices[k];
	md.radius = origin_radius;
	md.indices.assign(indices_count, indices_count + mesh_count);
	im->dirty = true;
	invalidate_slots(im);
	return LMX_OK;
}

int lmx_im_set_instances(LmxInstancedModels* im, uint32_t model, uint32_t n, const LmxImInstance* instances) {
	LMX_ENTER(im);
	if (model >= im->models.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown model %u (%zu registered)", model, im->models.size());
	if (n && !instances) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null instances");
	if ((uint64_t)n + im->total_instances - im->models[model].n > 0x7fffffffull) return fail(ctx, LMX_ERR_CAPACITY, "more than 2^31 instances");
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (int rc = im_relayout(im, model, n)) return rc;
	im->total_instances = im->total_instances - im->models[model].n + n;
	im->models[model].n = n;
	im->dirty = true;
	invalidate_slots(im);
	if (int rc = im_upload_tables(im)) return rc;
	LMX_HIP(ctx, upload_blocking(im->d_stage, instances, n));
	LMX_HIP(ctx, launch_im_grid_build(ctx->stream, im->d_stage.p, n, im->arrays(), im->table[model].first, im->d_grids.p + model));
	return LMX_OK;
}

int lmx_im_set_origins(LmxInstancedModels* im, uint32_t n_models, const double* pos_xyz) {
	LMX_ENTER(im);
	if (n_models > im->models.size() || (n_models && !pos_xyz)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%u origins for %zu models", n_models, im->models.size());
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	for (uint32_t m = 0; m < n_models; ++m)
		for (int k = 0; k < 3; ++k) im->models[m].origin[k] = pos_xyz[3 * (size_t)m + k];
	im->dirty = true;
	return LMX_OK;
}

int lmx_im_run(LmxInstancedModels* im, uint32_t view_slot, const LmxImView* view, const LmxShiftedFrustum* frustum) {
	LMX_ENTER(im);
	if (!view || !frustum) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null view / frustum");
	if (view_slot >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "view slot %u out of range (LMX_MAX_VIEWS = %d)", view_slot, LMX_MAX_VIEWS);
	if (im->dirty) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (int rc = im_upload_tables(im)) return rc;
	}
	LmxInstancedModels::Slot& s = im->slots[view_slot];
	const uint32_t nm = (uint32_t)im->models.size();
	Grow grow{ctx};
	if (int rc = grow(s.records, std::max<size_t>(2 * im->total_instances, 1))) return rc;
	if (int rc = grow(s.indirect, std::max<size_t>(im->n_indirect, 1))) return rc;
	if (int rc = grow(s.counts, std::max<size_t>(nm, 1))) return rc;
	if (!im->d_masks.p) LMX_HIP(ctx, im->d_masks.reserve(1));
	ImViewDev v;
	memset(&v, 0, sizeof(v));
	v.f = to_dev_frustum(*frustum);
	for (int k = 0; k < 3; ++k) v.cam[k] = view->camera_pos[k];
	v.lod_multiplier = view->lod_multiplier;
	v.time_delta = view->time_delta;
	v.is_shadow = view->is_shadow ? 1u : 0u;
	v.n_models = nm;
	const size_t half = im->d_model_tot.cap / 2; // (re-)allocated zero whenever the model count outgrows it; both halves hold 4 words per model
	uint32_t* tot = im->d_model_tot.p + im->tot_parity * half;
	uint32_t* tot_next = im->d_model_tot.p + (im->tot_parity ^ 1u) * half;
	LMX_HIP(ctx, launch_im_run(ctx->stream, im->d_models.p, im->d_grids.p, im->d_tile_model.p, im->n_tiles, v, im->arrays(), im->d_indices.p, im->d_masks.p,
		im->d_tile_counts.p, tot, tot_next, s.records.p, s.indirect.p, s.counts.p));
	im->tot_parity ^= 1u;
	s.valid = true;
	s.n_models = nm;
	s.n_indirect = im->n_indirect;
	return LMX_OK;
}

int lmx_im_read_grid(LmxInstancedModels* im, uint32_t model, LmxImGrid* out) {
	LMX_ENTER(im);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (model >= im->models.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown model %u", model);
	ImGridDev g;
	if (int rc = read_now(ctx, &g, (const ImGridDev*)im->d_grids.p + model, 1)) return rc;
	memset(out, 0, sizeof(*out));
	for (int k = 0; k < 3; ++k) {
		out->min[k] = g.mn[k];
		out->max[k] = g.mx[k];
	}
	out->placed = g.placed;
	out->unplaced = g.unplaced;
	for (int c = 0; c < LMX_IM_CELLS; ++c) {
		for (int k = 0; k < 3; ++k) {
			out->cells[c].min[k] = g.cmin[c][k];
			out->cells[c].max[k] = g.cmax[c][k];
		}
		out->cells[c].from_instance = g.from[c];
		out->cells[c].instance_count = g.count[c];
	}
	return LMX_OK;
}

int lmx_im_read_instances(LmxInstancedModels* im, uint32_t model, LmxImInstance* out, uint32_t cap) {
	LMX_ENTER(im);
	if (model >= im->models.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown model %u", model);
	const uint32_t n = im->models[model].n;
	if (cap < n) return fail(ctx, LMX_ERR_CAPACITY, "model %u holds %u instances, cap %u", model, n, cap);
	if (!n) return LMX_OK;
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (im->dirty) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (int rc = im_upload_tables(im)) return rc;
	}
	const size_t first = im->table[model].first;
	std::vector<float4> ps(n), rot(n);
	std::vector<float> lod(n);
	LMX_HIP(ctx, read_back(ps.data(), (const float4*)im->d_pos_scale.p + first, n, ctx->stream));
	LMX_HIP(ctx, read_back(rot.data(), (const float4*)im->d_rot.p + first, n, ctx->stream));
	if (int rc = read_now(ctx, lod.data(), (const float*)im->d_lod.p + first, n)) return rc;
	for (uint32_t i = 0; i < n; ++i) {
		out[i].rot[0] = rot[i].x; out[i].rot[1] = rot[i].y; out[i].rot[2] = rot[i].z;
		out[i].lod = lod[i];
		out[i].pos[0] = ps[i].x; out[i].pos[1] = ps[i].y; out[i].pos[2] = ps[i].z;
		out[i].scale = ps[i].w;
	}
	return LMX_OK;
}

int lmx_im_counts(LmxInstancedModels* im, uint32_t view_slot, LmxImCounts* out, uint32_t cap_models) {
	LMX_ENTER(im);
	if (int rc = im_check_slot(im, view_slot)) return rc;
	const LmxInstancedModels::Slot& s = im->slots[view_slot];
	static_assert(sizeof(ImCountsDev) == sizeof(LmxImCounts), "ImCountsDev mirrors LmxImCounts");
	return read_out(ctx, (ImCountsDev*)out, cap_models, (const ImCountsDev*)s.counts.p, s.n_models, s.n_models, "models' counts", NullOut::Refused);
}

int lmx_im_read_records(LmxInstancedModels* im, uint32_t view_slot, LmxImInstance* out, uint32_t cap, uint32_t* out_n) {
	LMX_ENTER(im);
	if (int rc = im_check_slot(im, view_slot)) return rc;
	const LmxInstancedModels::Slot& s = im->slots[view_slot];
	std::vector<LmxImCounts> c(std::max<uint32_t>(s.n_models, 1));
	if (int rc = lmx_im_counts(im, view_slot, c.data(), (uint32_t)c.size())) return rc;
	size_t total = 0;
	for (uint32_t m = 0; m < s.n_models; ++m) total += (size_t)c[m].bin_count[0] + c[m].bin_count[1] + c[m].bin_count[2] + c[m].bin_count[3];
	if (out_n) *out_n = (uint32_t)total;
	return read_out(ctx, out, cap, (const LmxImInstance*)s.records.p, total, total, "records", NullOut::Refused);
}

int lmx_im_read_indirect(LmxInstancedModels* im, uint32_t view_slot, LmxImIndirect* out, uint32_t cap, uint32_t* out_n) {
	LMX_ENTER(im);
	if (int rc = im_check_slot(im, view_slot)) return rc;
	const LmxInstancedModels::Slot& s = im->slots[view_slot];
	if (out_n) *out_n = s.n_indirect;
	return read_out(ctx, out, cap, (const LmxImIndirect*)s.indirect.p, s.n_indirect, s.n_indirect, "indirect records", NullOut::Refused);
}

int lmx_im_device_outputs(LmxInstancedModels* im, uint32_t view_slot, const void** d_records, const void** d_indirect, const void** d_counts) {
	if (!im) return LMX_ERR_INVALID_ARGUMENT;
	if (int rc = im_check_slot(im, view_slot)) return rc;
	const LmxInstancedModels::Slot& s = im->slots[view_slot];
	if (d_records) *d_records = s.records.p;
	if (d_indirect) *d_indirect = s.indirect.p;
	if (d_counts) *d_counts = s.counts.p;
	return LMX_OK;
}

} // extern "C"
