// lmx_capi_draw.hip — createCommands entry points (include/lumix_mi355.h, "draw commands" section): the tables the instance records
// need beyond the sort-key tables, the launch chain of draw_kernels.hip over the sorted pairs and the read-backs.
//
// The three sums of the chain (head flags -> run index, front bits -> decal ranks, slice sizes -> slice offsets) are hipcub device
// scans, as the instancer's offsets in lmx_capi_keys.hip: plain sums over n + 1 words are what the library does well; the one scan that is
// not a sum - the composition of the pairs' state functions - is the block-scan-with-carry of draw_kernels.hip.
#include "lmx_context.h"

#include <hipcub/hipcub.hpp>

using namespace lmx;

namespace {

// The temporary storage of the three sums (all over `n` words) is sized once, in front of the launch sequence.
int scan_reserve(LmxContext* ctx, size_t n, size_t* temp) {
	*temp = 0;
	LMX_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, *temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, ctx->stream));
	LMX_HIP(ctx, ctx->draw.d_scan_temp.reserve(std::max<size_t>(*temp, 1)));
	return LMX_OK;
}

int scan(LmxContext* ctx, const uint32_t* in, uint32_t* out, size_t n, size_t temp) {
	LMX_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ctx->draw.d_scan_temp.p, temp, in, out, (int)n, ctx->stream));
	return LMX_OK;
}

// The pass itself over n sorted pairs and an instancer CSR (n_groups groups, n_group_values renderables; n_groups == 0: none), all on the device.
int draw_pass(LmxContext* ctx, const LmxDrawView* view, uint32_t n_batches, const uint64_t* d_keys, const uint64_t* d_values, uint32_t n,
	const uint32_t* d_group_offset, const uint64_t* d_group_values, uint32_t n_groups, uint32_t n_group_values) {
	DrawState& ds = ctx->draw;
	KeysState& ks = ctx->keys;
	if (!view) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null view state");
	if (!n_batches) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "n_batches must be at least 1");
	if ((uint64_t)n * 96 + 16 > 0xffffffffull) return fail(ctx, LMX_ERR_CAPACITY, "%u pairs: the instance buffer's offsets are 32 bits", n);
	if ((uint64_t)n_group_values * 48 + 16 > 0xffffffffull) return fail(ctx, LMX_ERR_CAPACITY, "%u instanced renderables: the group buffer's offsets are 32 bits", n_group_values);
	DrawDevice d;
	memset(&d, 0, sizeof(d));
	if (int rc = bind_entity_transforms(ctx, d)) return rc;
	if (int rc = keys_upload_instances(ctx)) return rc; // as lmx_keys_run
	// ModelInstance::lod of the sorted set's entities lives in the slot-ordered mirror: hand it to the entity-indexed records the encode
	// reads (what lmx_keys_read_state does; the mirror stays valid)
	if (ks.mirror_valid)
		LMX_HIP(ctx, launch_keys_mirror_sync(ctx->stream, ctx->cull.ids.p, std::min(ks.mirror_slots, ctx->cull.n_padded), ks.d_inst_s.p, ks.soa().model,
			ks.mirror_split ? ks.d_state_s.p : nullptr, ks.d_inst.p, ks.n_entities));
	ds.ran = false;
	ds.n = n;
	ds.n_group_values = n_group_values;
	LMX_HIP(ctx, ds.d_counts.reserve(4));
	const size_t words = (size_t)n + 1, n_tiles = (n + DRAW_TILE - 1) / DRAW_TILE;
	LMX_HIP(ctx, ds.d_flags.reserve(words));
	LMX_HIP(ctx, ds.d_tile_fn.reserve(n_tiles + 1));
	LMX_HIP(ctx, ds.d_tile_in.reserve(n_tiles + 1));
	LMX_HIP(ctx, ds.d_words.reserve(7 * words));
	LMX_HIP(ctx, ds.d_runs.reserve(words));
	LMX_HIP(ctx, ds.d_instance_data.reserve((size_t)n * 96 + 16));
	LMX_HIP(ctx, ds.d_group_data.reserve((size_t)n_group_values * 48 + 16));
	size_t scan_temp = 0;
	if (int rc = scan_reserve(ctx, words, &scan_temp)) return rc;

	DrawViewDevice v;
	memset(&v, 0, sizeof(v));
	for (int k = 0; k < 3; ++k) { v.cam[k] = view->camera_pos[k]; v.origin[k] = view->frustum.origin[k]; }
	v.nx = view->frustum.xs[LMX_PLANE_NEAR]; v.ny = view->frustum.ys[LMX_PLANE_NEAR]; v.nz = view->frustum.zs[LMX_PLANE_NEAR]; v.nd = view->frustum.ds[LMX_PLANE_NEAR];
	for (uint32_t b = 0; b < 256; ++b) if (view->bucket_depth_sorted[b]) v.depth_sorted[b >> 5] |= 1u << (b & 31u);

	d.keys = d_keys; d.values = d_values; d.n = n;
	d.step = std::max<uint32_t>((uint32_t)(((uint64_t)n + n_batches - 1) / n_batches), 1u); // :2794
	if (n_groups) {
		d.group_offset = d_group_offset;
		d.group_values = d_group_values;
		d.n_groups = n_groups;
		d.n_group_values = n_group_values;
	}
	if (ks.have_instances) {
		d.inst = ks.d_inst.p; d.n_entities = std::min<uint32_t>(ks.n_entities, (uint32_t)ks.inst_uploaded);
		d.models = ks.d_models.p; d.n_models = (uint32_t)ks.models.size();
	}
	d.mesh_lod = ds.d_mesh_lod.p; d.n_meshes = ds.n_meshes;
	d.material_index = ds.d_material_index.p; d.n_mesh_materials = ds.n_material_index;
	d.prev = ds.d_prev.p; d.n_prev = ds.n_prev;
	d.bones_handle = ds.d_bones_handle.p; d.bones_offset = ds.d_bones_offset.p; d.n_bones = ds.n_bones;
	if (ds.have_decals) { d.decals = ds.d_decals.p; d.n_decals = ds.n_decals; }
	if (ds.have_curves) { d.curves = ds.d_curves.p; d.n_curves = ds.n_curves; }
	d.flags = ds.d_flags.p; d.tile_fn = ds.d_tile_fn.p; d.tile_in = ds.d_tile_in.p;
	uint32_t* w = ds.d_words.p;
	d.head = w; d.run_of = w + words; d.front = w + 2 * words; d.front_sum = w + 3 * words; d.run_start = w + 4 * words; d.run_bytes = w + 5 * words;
	d.run_offset = w + 6 * words;
	d.runs = ds.d_runs.p; d.instance_data = ds.d_instance_data.p; d.group_data = ds.d_group_data.p; d.counts = ds.d_counts.p;

	if (n) {
		LMX_HIP(ctx, hipMemsetAsync(d.run_bytes, 0, words * sizeof(uint32_t), ctx->stream)); // sizes behind the last run stay zero
		LMX_HIP(ctx, launch_draw_flags(ctx->stream, d, v));
		if (int rc = scan(ctx, d.head, d.run_of, words, scan_temp)) return rc;
		LMX_HIP(ctx, launch_draw_runs(ctx->stream, d, v));
		if (int rc = scan(ctx, d.front, d.front_sum, words, scan_temp)) return rc;
		if (int rc = scan(ctx, d.run_bytes, d.run_offset, words, scan_temp)) return rc;
		LMX_HIP(ctx, launch_draw_encode(ctx->stream, d, v));
	} else {
		const uint32_t zero[4] = {0, 0, 0, n_group_values};
		LMX_HIP(ctx, upload_on_stream(ds.d_counts.p, zero, 4, ctx->stream));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	LMX_HIP(ctx, launch_draw_groups(ctx->stream, d, v));
	ds.ran = true;
	return LMX_OK;
}

int host_counts(LmxContext* ctx, uint32_t c[4]) {
	if (!ctx->draw.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_draw_run has not run");
	return read_now(ctx, c, ctx->draw.d_counts.p, 4);
}

} // namespace

extern "C" {

int lmx_draw_set_meshes(LmxContext* ctx, const float* mesh_lod, uint32_t n_meshes) {
	LMX_CHECK_CTX(ctx);
	if (n_meshes && !mesh_lod) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null mesh table");
	if (int rc = upload_settled(ctx, ctx->draw.d_mesh_lod, mesh_lod, n_meshes)) return rc;
	ctx->draw.n_meshes = n_meshes;
	return LMX_OK;
}

int lmx_draw_set_material_indices(LmxContext* ctx, const uint32_t* material_index, uint32_t n_mesh_materials) {
	LMX_CHECK_CTX(ctx);
	if (n_mesh_materials && !material_index) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null material-index table");
	if (int rc = upload_settled(ctx, ctx->draw.d_material_index, material_index, n_mesh_materials)) return rc;
	ctx->draw.n_material_index = n_mesh_materials;
	return LMX_OK;
}

int lmx_draw_set_transforms(LmxContext* ctx, const LmxTransform* transforms, uint32_t n_entities) {
	LMX_CHECK_CTX(ctx);
	if (n_entities && !transforms) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null transforms");
	if (int rc = upload_settled(ctx, ctx->draw.d_tr, transforms, n_entities)) return rc;
	ctx->draw.n_tr = n_entities;
	return LMX_OK;
}

int lmx_draw_bind_world(LmxContext* ctx, int enable) {
	LMX_CHECK_CTX(ctx);
	ctx->draw.use_world = enable != 0;
	return LMX_OK;
}

int lmx_draw_set_prev_transforms(LmxContext* ctx, const LmxTransform* transforms, uint32_t n_entities) {
	LMX_CHECK_CTX(ctx);
	if (n_entities && !transforms) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null transforms");
	if (int rc = upload_settled(ctx, ctx->draw.d_prev, transforms, n_entities)) return rc;
	ctx->draw.n_prev = n_entities;
	return LMX_OK;
}

int lmx_draw_set_bones(LmxContext* ctx, const uint32_t* handle, const uint32_t* offset, uint32_t n_entities) {
	LMX_CHECK_CTX(ctx);
	if (n_entities && (!handle || !offset)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null bones table");
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ctx->draw.d_bones_handle, handle, n_entities, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ctx->draw.d_bones_offset, offset, n_entities, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ctx->draw.n_bones = n_entities;
	return LMX_OK;
}

int lmx_draw_set_decals(LmxContext* ctx, uint32_t n_entities, const float* half_extents, const float* uv_scale, const uint32_t* material_index,
	const float* curve_half_extents, const float* curve_uv_scale, const float* curve_bezier, const uint32_t* curve_material_index) {
	LMX_CHECK_CTX(ctx);
	const bool decals = half_extents || uv_scale || material_index, curves = curve_half_extents || curve_uv_scale || curve_bezier || curve_material_index;
	if (decals && !(half_extents && uv_scale && material_index)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the three decal tables come together");
	if (curves && !(curve_half_extents && curve_uv_scale && curve_bezier && curve_material_index)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the four curve-decal tables come together");
	DrawState& ds = ctx->draw;
	ds.have_decals = ds.have_curves = false;
	if (decals) {
		std::vector<DrawDecalRec> r(n_entities);
		for (uint32_t e = 0; e < n_entities; ++e) {
			memset(&r[e], 0, sizeof(DrawDecalRec));
			memcpy(r[e].half_extents, half_extents + 3 * (size_t)e, 12);
			memcpy(r[e].uv_scale, uv_scale + 2 * (size_t)e, 8);
			r[e].material_index = material_index[e];
		}
		if (int rc = upload_settled(ctx, ds.d_decals, r.data(), n_entities)) return rc;
		ds.n_decals = n_entities;
		ds.have_decals = true;
	}
	if (curves) {
		std::vector<DrawCurveRec> r(n_entities);
		for (uint32_t e = 0; e < n_entities; ++e) {
			memset(&r[e], 0, sizeof(DrawCurveRec));
			memcpy(r[e].half_extents, curve_half_extents + 3 * (size_t)e, 12);
			memcpy(r[e].uv_scale, curve_uv_scale + 2 * (size_t)e, 8);
			memcpy(r[e].bezier, curve_bezier + 4 * (size_t)e, 16);
			r[e].material_index = curve_material_index[e];
		}
		if (int rc = upload_settled(ctx, ds.d_curves, r.data(), n_entities)) return rc;
		ds.n_curves = n_entities;
		ds.have_curves = true;
	}
	return LMX_OK;
}

int lmx_draw_run(LmxContext* ctx, const LmxDrawView* view, uint32_t n_batches) {
	LMX_CHECK_CTX(ctx);
	KeysState& ks = ctx->keys;
	if (!ks.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_keys_run has not run");
	if (!ks.sorted) return fail(ctx, LMX_ERR_NOT_BUILT, "the pairs of the last lmx_keys_run are not sorted (lmx_keys_sort first)");
	return draw_pass(ctx, view, n_batches, ks.d_keys.p, ks.d_values.p, ks.n_sorted, ks.d_groups.p + ks.offsets_at, ks.d_group_values.p, ks.max_sort_key + 1, ks.n_sorted_recs);
}

int lmx_draw_run_pairs(LmxContext* ctx, const LmxDrawView* view, uint32_t n_batches, const uint64_t* keys, const uint64_t* values, uint32_t n,
	const uint32_t* group_offsets, const uint64_t* group_values, uint32_t n_groups) {
	LMX_CHECK_CTX(ctx);
	if (n && (!keys || !values)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null pairs");
	for (uint32_t i = 1; i < n; ++i)
		if (keys[i] < keys[i - 1]) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "pair %u: keys are not in ascending order", i);
	uint32_t n_group_values = 0;
	if (n_groups) {
		if (!group_offsets) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null group offsets");
		if (group_offsets[0] != 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "group offsets start at %u, not 0", group_offsets[0]);
		for (uint32_t k = 0; k < n_groups; ++k)
			if (group_offsets[k + 1] < group_offsets[k]) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "group %u: offsets descend", k);
		n_group_values = group_offsets[n_groups];
		if (n_group_values && !group_values) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null group values");
	}
	DrawState& ds = ctx->draw;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ds.d_keys, keys, n, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ds.d_values, values, n, ctx->stream));
	if (n_groups) {
		LMX_HIP(ctx, upload_on_stream(ds.d_group_offset, group_offsets, (size_t)n_groups + 1, ctx->stream));
		LMX_HIP(ctx, upload_on_stream(ds.d_group_values, group_values, n_group_values, ctx->stream));
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return draw_pass(ctx, view, n_batches, ds.d_keys.p, ds.d_values.p, n, ds.d_group_offset.p, ds.d_group_values.p, n_groups, n_group_values);
}

int lmx_draw_counts(LmxContext* ctx, LmxDrawCounts* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	uint32_t c[4];
	if (int rc = host_counts(ctx, c)) return rc;
	out->runs = c[0]; out->instance_bytes = c[1]; out->pairs = c[2]; out->group_records = c[3]; out->overflow = 0;
	return LMX_OK;
}

int lmx_draw_read_runs(LmxContext* ctx, LmxDrawRun* runs, uint32_t cap) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[4];
	if (int rc = host_counts(ctx, c)) return rc;
	return read_out(ctx, runs, cap, (const LmxDrawRun*)ctx->draw.d_runs.p, c[0], c[0], "runs");
}

int lmx_draw_read_instance_data(LmxContext* ctx, void* out, size_t cap_bytes) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[4];
	if (int rc = host_counts(ctx, c)) return rc;
	return read_out(ctx, (uint8_t*)out, cap_bytes, (const uint8_t*)ctx->draw.d_instance_data.p, c[1], c[1], "bytes");
}

int lmx_draw_read_group_data(LmxContext* ctx, void* out, size_t cap_bytes) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[4];
	if (int rc = host_counts(ctx, c)) return rc;
	const size_t bytes = (size_t)c[3] * 48;
	return read_out(ctx, (uint8_t*)out, cap_bytes, (const uint8_t*)ctx->draw.d_group_data.p, bytes, bytes, "bytes");
}

int lmx_draw_device_outputs(LmxContext* ctx, const LmxDrawRun** d_runs, const void** d_instance_data, const void** d_group_data, const uint32_t** d_counts) {
	LMX_CHECK_CTX(ctx);
	DrawState& ds = ctx->draw;
	if (!ds.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_draw_run has not run");
	if (d_runs) *d_runs = ds.d_runs.p;
	if (d_instance_data) *d_instance_data = ds.d_instance_data.p;
	if (d_group_data) *d_group_data = ds.d_group_data.p;
	if (d_counts) *d_counts = ds.d_counts.p;
	return LMX_OK;
}

} // extern "C"
