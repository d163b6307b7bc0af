// lmx_capi_world_edit.hip — lmx_world_edit / lmx_world_info (include/lumix_mi355.h): a batch of World::destroyEntity / createEntity /
// setParent applied to the world mirror where it lives. The host checks the batch against its mirror of `parent` (lmx_world_edit_host.h),
// the device derives the slot order again and moves the transforms old slot -> new slot into the second set of arrays
// (world_edit_kernels.hip); the two sets then trade places. What crosses the bus per call: the batch itself, one word per level, and
// one word per root for the cut of k_xform_subtree's run table. DESIGN.md 4.4.1.
#include "lmx_context.h"

#include <hipcub/hipcub.hpp>

using namespace lmx;

namespace {

// grow a buffer and keep its first `keep` elements (precondition: the stream was synchronized)
template <typename T> hipError_t grow_keep(DevBuf<T>& b, size_t n, size_t keep) {
	if (n <= b.cap) return hipSuccess;
	DevBuf<T> bigger;
	hipError_t e = bigger.reserve(n);
	if (e != hipSuccess) return e;
	e = device_copy_blocking(bigger.p, b.p, std::min(keep, b.cap));
	if (e != hipSuccess) return e;
	b.swap(bigger);
	return hipSuccess;
}

WorldDevice alt_dev(WorldState& w) {
	WorldDevice d;
	d.lpx = w.alt_pos[0].p; d.lpy = w.alt_pos[1].p; d.lpz = w.alt_pos[2].p; d.lrot = w.alt_rot[0].p; d.lsx = w.alt_scl[0].p; d.lsy = w.alt_scl[1].p; d.lsz = w.alt_scl[2].p;
	d.wpx = w.alt_pos[3].p; d.wpy = w.alt_pos[4].p; d.wpz = w.alt_pos[5].p; d.wrot = w.alt_rot[1].p; d.wsx = w.alt_scl[3].p; d.wsy = w.alt_scl[4].p; d.wsz = w.alt_scl[5].p;
	d.parent_slot = w.alt_parent_slot.p;
	d.dirty = w.d_dirty.p;
	return d;
}

// the hierarchy by entity on the device: stated from the mirror by the first edit after a build (4 + 1 bytes per entity, once)
int edit_device_state(LmxContext* ctx) {
	WorldState& w = ctx->world;
	if (w.edit_dev_valid) return LMX_OK;
	std::vector<int32_t> parent;
	std::vector<uint8_t> alive;
	w.mirror.resolve(&parent, &alive);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_blocking(w.d_parent, parent));
	LMX_HIP(ctx, upload_blocking(w.d_alive, alive));
	w.edit_dev_valid = true;
	return LMX_OK;
}

// k_xform_subtree's run table for the order just derived, cut as world_rebuild cuts it; n_sub_runs = 0 where the kernel's preconditions fail
int edit_run_table(LmxContext* ctx, uint32_t n_roots) {
	WorldState& w = ctx->world;
	const uint32_t n_levels = (uint32_t)w.level_start.size() - 1u;
	w.n_sub_runs = 0;
	if (!n_roots || n_levels < 1 || n_levels > XF_SUBTREE_MAX_LEVELS) return LMX_OK;
	LMX_HIP(ctx, upload_blocking(w.d_edit_level_start, w.level_start));
	LMX_HIP(ctx, w.d_edit_sizes.reserve(n_roots));
	LMX_HIP(ctx, launch_edit_root_sizes(ctx->stream, w.d_edit_root.p, w.d_edit_level_start.p, n_levels, n_roots, w.d_edit_sizes.p));
	std::vector<uint32_t> size(n_roots);
	LMX_HIP(ctx, read_back(size.data(), w.d_edit_sizes.p, n_roots, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<uint32_t> run_root;
	uint64_t heaviest = 0, in_run = 0;
	run_root.push_back(0);
	for (uint32_t r = 0; r < n_roots; ++r) {
		if (in_run && in_run + size[r] > XF_SUBTREE_NODES) { // close the run before this root
			run_root.push_back(r);
			heaviest = std::max(heaviest, in_run);
			in_run = 0;
		}
		in_run += size[r];
	}
	heaviest = std::max(heaviest, in_run);
	run_root.push_back(n_roots);
	if (heaviest > XF_SUBTREE_MAX_RUN) return LMX_OK;
	LMX_HIP(ctx, upload_blocking(w.d_edit_run_root, run_root));
	LMX_HIP(ctx, w.d_sub_table.reserve(run_root.size() * n_levels)); // (the stream is idle: no propagation reads the old table)
	LMX_HIP(ctx, launch_edit_run_table(ctx->stream, w.d_edit_root.p, w.d_edit_level_start.p, n_levels, w.d_edit_run_root.p, (uint32_t)run_root.size(), w.d_sub_table.p));
	w.n_sub_runs = (uint32_t)run_root.size() - 1u;
	return LMX_OK;
}

} // namespace

extern "C" {

int lmx_world_edit(LmxContext* ctx, uint32_t n_destroy, const int32_t* destroy_entity, uint32_t n_create, const int32_t* create_entity, const LmxTransform* create_transform,
	uint32_t n_reparent, const int32_t* new_parent, const int32_t* child) {
	LMX_CHECK_CTX(ctx);
	WorldState& w = ctx->world;
	if (!w.built) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_world_build has not been called");
	if (n_create && !create_transform) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null input array");
	if (int rc = edit_device_state(ctx)) return rc; // (the state of before the batch: the kill pass walks the old parents)
	WorldEditBatch batch;
	batch.n_destroy = n_destroy; batch.destroy_entity = destroy_entity;
	batch.n_create = n_create; batch.create_entity = create_entity;
	batch.n_reparent = n_reparent; batch.new_parent = new_parent; batch.child = child;
	std::vector<int32_t> rp_child, rp_parent;
	uint32_t which = 0;
	const uint32_t n_old = w.n;
	WorldEditUndo undo;
	if (const char* why = world_edit_check_apply(w.mirror, batch, &rp_child, &rp_parent, &which, &undo)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%s (list entry %u)", why, which);
	const bool drop = n_destroy && !w.bound_entity.empty(); // bindings may die with their entities
	// The batch is accepted. The reference propagates every write before the next call: what was staged goes first (its moved list
	// stays in the buffers), on the world of before the batch - the batch comes out of the mirror for it and goes in again. A
	// propagation also states the binding tables on the device where a new binding or a rebuild left them unstated: the pass that finds
	// the dropped bindings reads them. Where it states them, it leaves the entries of the entities this batch kills void (the engine
	// may have taken those out of the culling system already) and lists them in edit_skipped; the device pass below cannot see those.
	w.edit_skipped.clear();
	if (w.pending || (drop && w.bound_generation == ~0ull)) {
		world_edit_rollback(w.mirror, undo);
		w.edit_doomed.assign(destroy_entity, destroy_entity + n_destroy);
		std::sort(w.edit_doomed.begin(), w.edit_doomed.end());
		w.edit_in_flight = true;
		const int rc = lmx_world_propagate(ctx);
		w.edit_in_flight = false;
		if (rc) {
			if (!w.edit_skipped.empty()) w.bound_generation = ~0ull; // (the tables may hold void entries of entities that live on)
			return rc;
		}
		if (world_edit_check_apply(w.mirror, batch, &rp_child, &rp_parent, &which, &undo)) {
			if (!w.edit_skipped.empty()) w.bound_generation = ~0ull;
			return fail(ctx, LMX_ERR_INVALID, "lmx_world_edit: the batch was accepted and is refused after the propagation");
		}
	}
	// The mirror now states the world after the batch. Until the two sets of arrays trade places a failure of any step below takes the
	// batch back out of it, and the device's copy of `parent` (partly edited by then) is stated again from the mirror by the next edit;
	// so are the binding tables, where entries were left void for this batch.
	struct Guard {
		WorldState& w;
		const WorldEditUndo& undo;
		bool armed = true;
		~Guard() {
			if (!armed) return;
			world_edit_rollback(w.mirror, undo);
			w.edit_dev_valid = false;
			if (!w.edit_skipped.empty()) w.bound_generation = ~0ull;
		}
	} guard{w, undo};
	const uint32_t n = w.mirror.n();
	if (!n || !(n_destroy + n_create + n_reparent)) {
		guard.armed = false;
		++w.edits;
		return LMX_OK;
	}
	hipStream_t st = ctx->stream;
	LMX_HIP(ctx, hipStreamSynchronize(st));

	// ---- the batch, by entity ----
	if (n > n_old) {
		LMX_HIP(ctx, grow_keep(w.d_parent, n, n_old));
		LMX_HIP(ctx, grow_keep(w.d_alive, n, n_old));
		LMX_HIP(ctx, hipMemsetAsync(w.d_parent.p + n_old, 0xff, (size_t)(n - n_old) * sizeof(int32_t), st));
		LMX_HIP(ctx, hipMemsetAsync(w.d_alive.p + n_old, 0, n - n_old, st));
		if (w.track_moved) { // the lists hold two propagations of the grown world; the entries already there stay readable
			LMX_HIP(ctx, grow_keep(w.d_moved_entity, (size_t)n * 2, (size_t)n_old * 2));
			LMX_HIP(ctx, grow_keep(w.d_moved_tr, (size_t)n * 2, (size_t)n_old * 2));
		}
	}
	LMX_HIP(ctx, w.d_edit_mark.reserve(n));
	LMX_HIP(ctx, w.d_edit_kill.reserve(n));
	LMX_HIP(ctx, hipMemsetAsync(w.d_edit_mark.p, 0, n, st));
	LMX_HIP(ctx, hipMemsetAsync(w.d_edit_kill.p, 0, n, st));
	LMX_HIP(ctx, upload_blocking(w.d_edit_destroy, destroy_entity, n_destroy));
	LMX_HIP(ctx, upload_blocking(w.d_edit_create, create_entity, n_create));
	LMX_HIP(ctx, upload_blocking(w.d_edit_tr, create_transform, n_create));
	LMX_HIP(ctx, upload_blocking(w.d_edit_child, rp_child));
	LMX_HIP(ctx, upload_blocking(w.d_edit_new_parent, rp_parent));
	WorldEditDevice ed;
	ed.parent = w.d_parent.p; ed.alive = w.d_alive.p; ed.mark = w.d_edit_mark.p; ed.kill = w.d_edit_kill.p;
	LMX_HIP(ctx, w.d_edit_word.reserve(3)); // [0] live entities, [1] a small level's total, [2] dropped bindings
	LMX_HIP(ctx, hipMemsetAsync(w.d_edit_word.p, 0, 3 * sizeof(uint32_t), st));
	LMX_HIP(ctx, launch_edit_kill(st, ed, w.d_edit_destroy.p, n_destroy, n_old));
	const uint32_t n_bound = drop && w.bound_generation != ~0ull ? (uint32_t)w.bound_entity.size() : 0u;
	if (n_bound) { // which entries of the host's binding list die: a handful of indices come back, not the list
		LMX_HIP(ctx, w.d_edit_dropped.reserve(n_bound));
		LMX_HIP(ctx, launch_edit_dropped(st, w.d_entity_of_slot.p, w.d_edit_kill.p, w.d_bound_slot.p, n_bound, w.d_edit_dropped.p, w.d_edit_word.p + 2));
	}
	LMX_HIP(ctx, launch_edit_link(st, ed, w.d_edit_create.p, n_create, w.d_edit_child.p, w.d_edit_new_parent.p, (uint32_t)rp_child.size()));

	// ---- the order: children grouped by parent, then level by level from the roots ----
	LMX_HIP(ctx, w.d_edit_key.reserve(n));
	LMX_HIP(ctx, w.d_edit_key_alt.reserve(n));
	LMX_HIP(ctx, w.d_edit_val.reserve(n));
	LMX_HIP(ctx, w.d_edit_val_alt.reserve(n));
	LMX_HIP(ctx, w.d_edit_first.reserve((size_t)n + 1));
	LMX_HIP(ctx, w.d_edit_count.reserve((size_t)n + 1));
	LMX_HIP(ctx, w.d_edit_root.reserve(n));
	LMX_HIP(ctx, w.d_edit_cnt.reserve((size_t)n + 1));
	LMX_HIP(ctx, w.d_edit_off.reserve((size_t)n + 1));
	LMX_HIP(ctx, w.alt_parent_slot.reserve(n));
	LMX_HIP(ctx, w.alt_slot_of_entity.reserve(n));
	LMX_HIP(ctx, w.alt_entity_of_slot.reserve(n));
	LMX_HIP(ctx, hipMemsetAsync(w.d_edit_first.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
	LMX_HIP(ctx, hipMemsetAsync(w.d_edit_count.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
	LMX_HIP(ctx, launch_edit_keys(st, ed, n, w.d_edit_key.p, w.d_edit_val.p, w.d_edit_word.p));
	{
		int bits = 1;
		while (bits < 32 && (n >> bits) != 0) ++bits; // keys are parent + 1 <= n
		size_t temp = 0;
		LMX_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, temp, w.d_edit_key.p, w.d_edit_key_alt.p, w.d_edit_val.p, w.d_edit_val_alt.p, (int)n, 0, bits, st));
		size_t scan_temp = 0;
		LMX_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n + 1), st));
		LMX_HIP(ctx, w.d_edit_temp.reserve(std::max(temp, scan_temp)));
		LMX_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(w.d_edit_temp.p, temp, w.d_edit_key.p, w.d_edit_key_alt.p, w.d_edit_val.p, w.d_edit_val_alt.p, (int)n, 0, bits, st));
	}
	LMX_HIP(ctx, launch_edit_child_ranges(st, w.d_edit_key_alt.p, n, w.d_edit_first.p, w.d_edit_count.p));
	uint32_t n_roots = 0, n_live = 0, n_dropped = 0;
	LMX_HIP(ctx, read_back(&n_roots, w.d_edit_count.p, 1, st));
	LMX_HIP(ctx, read_back(&n_live, w.d_edit_word.p, 1, st));
	LMX_HIP(ctx, read_back(&n_dropped, w.d_edit_word.p + 2, 1, st));
	LMX_HIP(ctx, hipStreamSynchronize(st));
	if (!n_roots || n_dropped > n_bound) return fail(ctx, LMX_ERR_INVALID, "lmx_world_edit: %u roots, %u of %u bindings dropped", n_roots, n_dropped, n_bound);
	std::vector<uint32_t> dropped(n_dropped);
	LMX_HIP(ctx, read_back(dropped.data(), w.d_edit_dropped.p, n_dropped, st)); // (lands with the first level's wait below)
	WorldEditOrder o;
	o.sorted = w.d_edit_val_alt.p; o.first = w.d_edit_first.p; o.count = w.d_edit_count.p;
	o.entity_of_slot = w.alt_entity_of_slot.p; o.slot_of_entity = w.alt_slot_of_entity.p; o.parent_slot = w.alt_parent_slot.p; o.root_of_slot = w.d_edit_root.p;
	LMX_HIP(ctx, launch_edit_roots(st, o, n_roots));
	std::vector<uint32_t> level_start;
	level_start.push_back(0);
	level_start.push_back(n_roots);
	for (uint32_t first = 0, m = n_roots; m != 0;) { // one host wait per level: the next level's size
		uint32_t total = 0;
		if (m <= WORLD_EDIT_SMALL_LEVEL) {
			LMX_HIP(ctx, launch_edit_level_small(st, o, first, m, w.d_edit_word.p + 1));
			LMX_HIP(ctx, read_back(&total, w.d_edit_word.p + 1, 1, st));
		} else {
			LMX_HIP(ctx, launch_edit_level_count(st, o, first, m, w.d_edit_cnt.p));
			size_t temp = w.d_edit_temp.cap;
			LMX_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(w.d_edit_temp.p, temp, w.d_edit_cnt.p, w.d_edit_off.p, (int)(m + 1), st));
			LMX_HIP(ctx, launch_edit_level_scatter(st, o, first, m, w.d_edit_cnt.p, w.d_edit_off.p));
			LMX_HIP(ctx, read_back(&total, w.d_edit_off.p + m, 1, st));
		}
		LMX_HIP(ctx, hipStreamSynchronize(st));
			if ((uint64_t)level_start.back() + total > n) return fail(ctx, LMX_ERR_INVALID, "lmx_world_edit: the level expansion ran past %u entities", n);
		first += m;
		m = total;
		if (m) level_start.push_back(level_start.back() + m);
	}
	if (level_start.back() != n) return fail(ctx, LMX_ERR_INVALID, "lmx_world_edit: %u of %u entities reachable from the roots", level_start.back(), n);

	// ---- the transforms and every table that names slots: old slot -> new slot, into the second set ----
	for (auto& b : w.alt_pos) LMX_HIP(ctx, b.reserve(n));
	for (auto& b : w.alt_rot) LMX_HIP(ctx, b.reserve(n));
	for (auto& b : w.alt_scl) LMX_HIP(ctx, b.reserve(n));
	const bool tables = !w.bound_entity.empty() && w.bound_generation != ~0ull; // the device binding tables are stated (world_upload_binding)
	if (tables) {
		LMX_HIP(ctx, w.alt_bound_dyn_of_slot.reserve(n));
		LMX_HIP(ctx, w.alt_bound_radius_of_slot.reserve(n));
	}
	if (w.d_dirty.cap < n) LMX_HIP(ctx, w.d_dirty.reserve(n)); // (every mark is clear: the propagation above, or nothing staged)
	LMX_HIP(ctx, hipMemsetAsync(w.d_dirty.p, 0, n, st));
	const WorldDevice to = alt_dev(w);
	LMX_HIP(ctx, launch_edit_permute(st, w.dev(), to, w.alt_entity_of_slot.p, w.d_slot_of_entity.p, w.d_edit_kill.p, n_old, n, w.d_bound_dyn_of_slot.p,
		w.d_bound_radius_of_slot.p, tables ? w.alt_bound_dyn_of_slot.p : nullptr, tables ? w.alt_bound_radius_of_slot.p : nullptr));
	LMX_HIP(ctx, launch_edit_create(st, to, w.alt_slot_of_entity.p, w.d_edit_create.p, w.d_edit_tr.p, n_create));
	LMX_HIP(ctx, launch_edit_locals(st, to, w.alt_slot_of_entity.p, w.d_edit_child.p, w.d_edit_new_parent.p, (uint32_t)rp_child.size()));
	// the last launch, as it alone rewrites tables of the set in use in place: after it nothing is left that can fail before the flip
	LMX_HIP(ctx, launch_edit_remap(st, w.d_entity_of_slot.p, w.alt_slot_of_entity.p, w.d_edit_kill.p, w.d_bound_slot.p, tables ? (uint32_t)w.bound_entity.size() : 0u,
		w.d_attach.p, w.attach_invalidated ? 0u : w.n_attach));
	// the sets trade places: every consumer reads ctx->world's pointers when it launches
	guard.armed = false;
	++w.edits;
	for (uint32_t i : dropped) w.bound_entity[i] = -1; // (the entry stays, void, so that the list keeps step with the device's)
	for (uint32_t i : w.edit_skipped) w.bound_entity[i] = -1; // (void on the device since the propagation above stated the tables)
	w.edit_skipped.clear();
	for (int i = 0; i < 6; ++i) w.pos[i].swap(w.alt_pos[i]);
	for (int i = 0; i < 2; ++i) w.rot[i].swap(w.alt_rot[i]);
	for (int i = 0; i < 6; ++i) w.scl[i].swap(w.alt_scl[i]);
	w.d_parent_slot.swap(w.alt_parent_slot);
	w.d_slot_of_entity.swap(w.alt_slot_of_entity);
	w.d_entity_of_slot.swap(w.alt_entity_of_slot);
	if (tables) {
		w.d_bound_dyn_of_slot.swap(w.alt_bound_dyn_of_slot);
		w.d_bound_radius_of_slot.swap(w.alt_bound_radius_of_slot);
	}
	w.n = n;
	w.n_live = n_live;
	w.level_start.swap(level_start);
	w.slot_of_entity.resize(n);
	w.entity_of_slot.resize(n);
	w.parent_slot.resize(n);
	w.host_slots_stale = true;
	return edit_run_table(ctx, n_roots);
}

int lmx_world_info(LmxContext* ctx, LmxWorldInfo* out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	const WorldState& w = ctx->world;
	if (!w.built) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_world_build has not been called");
	memset(out, 0, sizeof(*out));
	out->n = w.n;
	out->n_live = w.n_live;
	out->n_levels = (uint32_t)w.level_start.size() - 1u;
	out->fused = w.fused_levels && w.n_sub_runs ? 1u : 0u;
	out->edits = w.edits;
	return LMX_OK;
}

} // extern "C"
