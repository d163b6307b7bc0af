// lmx_capi_poses.hip — PoseProcessor entry points (include/lumix_mi355.h, "pose processor" section): the skin instance of every entity, the
// frame's dual-quaternion buffer with its cursor on the device, the launch chain of pose_kernels.hip over the pose list of the last
// lmx_keys_run (or a caller's list) and the read-backs. lmx_poses_run enqueues and returns: the list's length never reaches the host.
#include "lmx_context.h"

using namespace lmx;

namespace {

// The frame's buffer holds every instance's dual quaternions once (an instance is handed over at most once per frame) + the guard behind
// them. (Re)reserved when the skin instance table changed since: the frame then starts over.
int poses_reserve(LmxContext* ctx) {
	PosesState& ps = ctx->poses;
	SkinState& sk = ctx->skin;
	if (ps.reserved_bones == sk.bones_total) return LMX_OK;
	if ((uint64_t)sk.bones_total * POSE_BONE_BYTES > 0xf0000000ull) return fail(ctx, LMX_ERR_CAPACITY, "%zu bones: the slices' offsets are 32 bits", sk.bones_total);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, ps.d_dual_quats.reserve(sk.bones_total * 2 + POSES_GUARD_BYTES / sizeof(float4)));
	LMX_HIP(ctx, ps.d_state.reserve(POSES_STATE_WORDS));
	LMX_HIP(ctx, ps.d_block_sum.reserve(POSE_GRID));
	LMX_HIP(ctx, fill_guard(ps.d_dual_quats.p + sk.bones_total * 2, POSES_GUARD_BYTES / sizeof(float4), ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps.d_state.p, 0, POSES_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	ps.cap_bytes = (uint32_t)(sk.bones_total * POSE_BONE_BYTES);
	ps.reserved_bones = sk.bones_total;
	return LMX_OK;
}

// The draw encoder's pose->slice tables cover the entities of lmx_poses_set_instances: grown here when lmx_draw_set_bones uploaded fewer
// (or never did), what they hold is kept, the new entries read as zero.
int poses_grow_tables(LmxContext* ctx) {
	PosesState& ps = ctx->poses;
	DrawState& ds = ctx->draw;
	if (ds.n_bones >= ps.n_entities && ds.d_bones_handle.p && ds.d_bones_offset.p) return LMX_OK;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const size_t n = std::max<size_t>(ps.n_entities, 1), keep = std::min<size_t>(ds.n_bones, n);
	for (DevBuf<uint32_t>* t : {&ds.d_bones_handle, &ds.d_bones_offset}) {
		DevBuf<uint32_t> grown;
		LMX_HIP(ctx, grown.reserve(n));
		LMX_HIP(ctx, hipMemsetAsync(grown.p, 0, n * sizeof(uint32_t), ctx->stream));
		if (t->p) LMX_HIP(ctx, device_copy_on_stream(grown.p, t->p, keep, ctx->stream));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		t->swap(grown);
	}
	ds.n_bones = std::max(ds.n_bones, ps.n_entities);
	return LMX_OK;
}

int poses_ready(LmxContext* ctx) {
	if (!ctx->poses.have_instances) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_poses_set_instances has not been called");
	return LMX_OK;
}

// The pass over `list_cap` entries at most of `d_list`, its length on the device.
int poses_pass(LmxContext* ctx, const int32_t* d_list, const uint32_t* d_count, size_t list_cap) {
	PosesState& ps = ctx->poses;
	SkinState& sk = ctx->skin;
	if (sk.inst.empty()) return fail(ctx, LMX_ERR_NOT_BUILT, "no skin instances (lmx_skin_set_instances)");
	if (!sk.pose_is_absolute) return fail(ctx, LMX_ERR_NOT_BUILT, "no absolute poses: lmx_skin_run has not run, or pose write-back is disabled (computeSkeletonDualQuats: ASSERT(pose.is_absolute))");
	if (int rc = poses_reserve(ctx)) return rc;
	if (int rc = poses_grow_tables(ctx)) return rc;
	list_cap = std::min<size_t>(list_cap, 1u << 31);
	if (int rc = Grow{ctx}(ps.d_entries, list_cap)) return rc; // (a pass of the previous view may still read the old records)
	PosesDevice d;
	memset(&d, 0, sizeof(d));
	d.list = d_list; d.list_count = d_count; d.list_cap = (uint32_t)list_cap;
	d.skin_of_entity = ps.d_skin_of_entity.p; d.n_entities = ps.n_entities;
	d.inst = sk.d_inst.p; d.n_inst = (uint32_t)sk.inst.size();
	d.pose_pos = sk.d_pose_pos.p; d.pose_rot = sk.d_pose_rot.p; d.inv_pos = sk.d_inv_pos.p; d.inv_rot = sk.d_inv_rot.p;
	d.entries = ps.d_entries.p; d.block_sum = ps.d_block_sum.p; d.state = ps.d_state.p;
	d.dual_quats = ps.d_dual_quats.p; d.cap_bytes = ps.cap_bytes;
	d.handle = ps.handle; d.base_offset = ps.base_offset;
	d.bones_handle = ctx->draw.d_bones_handle.p; d.bones_offset = ctx->draw.d_bones_offset.p; d.n_table = std::min(ctx->draw.n_bones, ps.n_entities);
	ProfScope prof(ctx, LMX_K_POSE_SLICES);
	LMX_HIP(ctx, launch_pose_slices(ctx->stream, d));
	LMX_HIP(ctx, launch_pose_dual_quats(ctx->stream, d));
	return LMX_OK;
}

int host_counts(LmxContext* ctx, uint32_t c[4]) {
	if (int rc = poses_ready(ctx)) return rc;
	if (int rc = poses_reserve(ctx)) return rc;
	return read_now(ctx, c, ctx->poses.d_state.p, 4);
}

} // namespace

extern "C" {

int lmx_poses_set_instances(LmxContext* ctx, uint32_t n_entities, const int32_t* skin_instance) {
	LMX_CHECK_CTX(ctx);
	if (n_entities && !skin_instance) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null skin instance table");
	PosesState& ps = ctx->poses;
	if (int rc = upload_settled(ctx, ps.d_skin_of_entity, skin_instance, n_entities)) return rc;
	ps.n_entities = n_entities;
	ps.have_instances = true;
	ps.reserved_bones = ~(size_t)0; // the frame starts over
	if (int rc = poses_reserve(ctx)) return rc;
	return poses_grow_tables(ctx);
}

int lmx_poses_begin_frame(LmxContext* ctx, uint32_t handle, uint32_t base_offset) {
	LMX_CHECK_CTX(ctx);
	if (int rc = poses_ready(ctx)) return rc;
	if (int rc = poses_reserve(ctx)) return rc;
	PosesState& ps = ctx->poses;
	if ((uint64_t)base_offset + ps.cap_bytes > 0xffffffffull) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "base offset %u + %u bytes of slices pass 32 bits", base_offset, ps.cap_bytes);
	LMX_HIP(ctx, hipMemsetAsync(ps.d_state.p, 0, POSES_STATE_WORDS * sizeof(uint32_t), ctx->stream));
	ps.handle = handle;
	ps.base_offset = base_offset;
	return LMX_OK;
}

int lmx_poses_run(LmxContext* ctx) {
	LMX_CHECK_CTX(ctx);
	if (int rc = poses_ready(ctx)) return rc;
	KeysState& ks = ctx->keys;
	if (!ks.ran) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_keys_run has not run");
	// (an entity is listed once per frame and every listed entity has an instance record: the list is no longer than the record table)
	return poses_pass(ctx, ks.d_poses.p, ks.d_groups.p + ks.counters_at + KEYS_N_POSES, std::min<size_t>(ks.d_poses.cap, ks.n_entities));
}

int lmx_poses_run_list(LmxContext* ctx, const int32_t* entities, uint32_t n) {
	LMX_CHECK_CTX(ctx);
	if (int rc = poses_ready(ctx)) return rc;
	if (n && !entities) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null list");
	PosesState& ps = ctx->poses;
	if (int rc = poses_reserve(ctx)) return rc;
	if (int rc = upload_list(ctx, ps.d_list, entities, n, ps.d_state.p + POSES_LIST_N, ps.list_n)) return rc;
	return poses_pass(ctx, ps.d_list.p, ps.d_state.p + POSES_LIST_N, n);
}

int lmx_poses_counts(LmxContext* ctx, LmxPosesCounts* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	uint32_t c[4];
	if (int rc = host_counts(ctx, c)) return rc;
	out->instances = c[POSES_INSTANCES]; out->bytes = c[POSES_BYTES]; out->skipped = c[POSES_SKIPPED]; out->overflow = c[POSES_OVERFLOW];
	return LMX_OK;
}

int lmx_poses_read_slices(LmxContext* ctx, uint32_t* handle, uint32_t* offset, uint32_t n_entities) {
	LMX_CHECK_CTX(ctx);
	if (int rc = poses_ready(ctx)) return rc;
	PosesState& ps = ctx->poses;
	if (n_entities < ps.n_entities) return fail(ctx, LMX_ERR_CAPACITY, "need room for %u entities", ps.n_entities);
	if (int rc = poses_grow_tables(ctx)) return rc;
	LMX_HIP(ctx, read_back(handle, ctx->draw.d_bones_handle.p, ps.n_entities, ctx->stream));
	return read_now(ctx, offset, (const uint32_t*)ctx->draw.d_bones_offset.p, ps.n_entities);
}

int lmx_poses_read_buffer(LmxContext* ctx, void* out, size_t cap_bytes) {
	LMX_CHECK_CTX(ctx);
	uint32_t c[4];
	if (int rc = host_counts(ctx, c)) return rc;
	return read_out(ctx, (uint8_t*)out, cap_bytes, (const uint8_t*)ctx->poses.d_dual_quats.p, c[POSES_BYTES], (size_t)ctx->poses.cap_bytes + POSES_GUARD_BYTES, "bytes");
}

int lmx_poses_device_outputs(LmxContext* ctx, const void** d_dual_quats, const uint32_t** d_counts) {
	LMX_CHECK_CTX(ctx);
	if (int rc = poses_ready(ctx)) return rc;
	if (int rc = poses_reserve(ctx)) return rc;
	if (d_dual_quats) *d_dual_quats = ctx->poses.d_dual_quats.p;
	if (d_counts) *d_counts = ctx->poses.d_state.p;
	return LMX_OK;
}

} // extern "C"
