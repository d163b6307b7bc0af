// lmx_capi_cull_set.hip — the host mirror of the culling system's two resident sets (see lmx_capi_cull.hip) and its O(1) mutations,
// with the entry points that use nothing else: add / remove / set*, their batched forms, bind / unbind. No HIP call is made here except
// through cull_dyn_sync_mirror (one read-back, lmx_capi_cull.hip). The _impl functions, the batched loops and the replay of the
// asynchronous compaction's operation log share this unit so that the compiler inlines the former into the latter two.
#include "lmx_cull_host.h"

using namespace lmx;

namespace {

// ---- dynamic set: slots and patches (queue_dyn_patch: below, the asynchronous compaction's swap calls it too) ----
uint32_t take_dyn_slot(CullSet& cs, uint8_t type) {
	if (cs.dyn_layout_dirty) return DYN_NO_SLOT;
	if (!cs.dyn_free[type].empty()) {
		const uint32_t s = cs.dyn_free[type].back();
		cs.dyn_free[type].pop_back();
		return s;
	}
	if (cs.dyn_next[type] < cs.dyn_tt.ent_end[type]) return cs.dyn_next[type]++;
	cs.dyn_layout_dirty = true; // region full: the next flush reassigns every slot with more room
	return DYN_NO_SLOT;
}

void dyn_append(CullSet& cs, int32_t entity, uint8_t type, DV3 pos, float radius, bool bound) {
	if ((size_t)entity >= cs.ent_to_dyn.size()) cs.ent_to_dyn.resize((size_t)entity + 1, -1);
	cs.ent_to_dyn[entity] = (int32_t)cs.dyn.size();
	DynRec r{{pos.x, pos.y, pos.z}, radius, entity, take_dyn_slot(cs, type), type, bound};
	cs.dyn.push_back(r);
	if (!bound) cs.n_unbound++;
	queue_dyn_patch(cs, r, true);
}

void remove_dynamic(CullSet& cs, uint32_t idx) {
	const DynRec r = cs.dyn[idx];
	queue_dyn_patch(cs, r, false);
	if (r.slot != DYN_NO_SLOT && !cs.dyn_layout_dirty) cs.dyn_free[r.type].push_back(r.slot);
	if (!r.bound) cs.n_unbound--;
	const uint32_t last = (uint32_t)cs.dyn.size() - 1;
	if (idx != last) {
		cs.dyn[idx] = cs.dyn[last];
		cs.ent_to_dyn[cs.dyn[idx].entity] = (int32_t)idx;
	}
	cs.dyn.pop_back();
	cs.ent_to_dyn[r.entity] = -1;
}

// ---- static set: host mirror ops --------------------------------------------------------------------------------
void remove_static(CullSet& cs, uint32_t rec) { // culling_system.cpp:160-190: the device slot becomes a tombstone
	const int32_t entity = cs.recs[rec].entity;
	if (layout_live(cs)) {
		cs.q_id.push_back(PatchId{cs.rec_slot[rec], -1});
		cs.n_tombstones++;
	}
	const uint32_t last = (uint32_t)cs.recs.size() - 1;
	if (rec != last) {
		cs.recs[rec] = cs.recs[last];
		cs.ent_to_rec[cs.recs[rec].entity] = (int32_t)rec;
		if (layout_live(cs)) cs.rec_slot[rec] = cs.rec_slot[last];
	}
	cs.recs.pop_back();
	if (layout_live(cs)) cs.rec_slot.pop_back();
	cs.ent_to_rec[entity] = -1;
}

// remove(entity); add(entity, type, pos, radius) of culling_system.cpp:201-258 when the cell or the big flag changes
void readd_static(CullSet& cs, uint32_t rec, DV3 pos, float radius) {
	const CullRec old = cs.recs[rec];
	if (!layout_live(cs)) {
		cs.recs[rec] = make_cull_rec(old.entity, old.type, pos, radius);
		return;
	}
	remove_static(cs, rec);
	dyn_append(cs, old.entity, old.type, pos, radius, false);
}

void mark_patch(CullSet& cs, uint32_t rec) {
	if (!layout_live(cs)) return;
	const CullRec& r = cs.recs[rec];
	const PatchSphere p{cs.rec_slot[rec], r.rel.x, r.rel.y, r.rel.z, r.radius};
	if (cs.q_sphere_at.size() < cs.n_padded) cs.q_sphere_at.resize(cs.n_padded, ~0u);
	uint32_t& at = cs.q_sphere_at[p.slot];
	if (at != ~0u) { // set twice before the next flush: the last write wins
		cs.q_sphere[at] = p;
		return;
	}
	at = (uint32_t)cs.q_sphere.size();
	cs.q_sphere.push_back(p);
}

// What the reference's stored state (cell, cell-relative fp32 position) means as a world position:
// cell.header.origin + sphere->position (culling_system.cpp:255)
DV3 stored_position(DV3 pos) {
	const IV3 idx = cell_of(pos);
	const DV3 origin = cell_origin(idx);
	return add(origin, to_v3(sub(pos, origin)));
}

// ---- the mutating operations, on a given set ------------------------------------------------------------------------------------
// `cs` is the context's live set for the public entry points and the SHADOW set when the asynchronous compaction replays the
// operation log (replay = true: no device round trips, and LMX_CULL_OPT_DEVICE_OWNS_BOUND - a statement about the live device set at
// the time of the call - is not consulted: only operations that took effect are logged). `*effective` = the set changed.
static int cull_add_impl(LmxContext* ctx, CullSet& cs, int32_t entity, uint8_t type, const double pos[3], float radius) { // culling_system.cpp:131-157
	if (entity < 0 || !pos) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad entity/pos");
	if (type >= MAX_TYPES) return fail(ctx, LMX_ERR_CAPACITY, "type %u >= LMX_MAX_TYPES", type);
	uint32_t idx;
	if (locate(cs, entity, &idx) != Where::NONE) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %d already added", entity);
	if (layout_live(cs)) {
		dyn_append(cs, entity, type, DV3{pos[0], pos[1], pos[2]}, radius, false); // sorted in by the next compaction
		return LMX_OK;
	}
	if ((size_t)entity >= cs.ent_to_rec.size()) cs.ent_to_rec.resize((size_t)entity + 1, -1);
	cs.ent_to_rec[entity] = (int32_t)cs.recs.size();
	cs.recs.push_back(make_cull_rec(entity, type, DV3{pos[0], pos[1], pos[2]}, radius));
	cs.structure_dirty = true;
	return LMX_OK;
}

static int cull_remove_impl(CullSet& cs, int32_t entity, bool* effective) { // culling_system.cpp:160-190 (unknown entities are ignored, :162-165)
	uint32_t idx;
	*effective = true;
	switch (locate(cs, entity, &idx)) {
		case Where::STATIC: remove_static(cs, idx); break;
		case Where::DYNAMIC: remove_dynamic(cs, idx); break;
		case Where::NONE: *effective = false; break;
	}
	return LMX_OK;
}

static int cull_set_impl(LmxContext* ctx, CullSet& cs, bool device_owns_bound, int32_t entity, const double pos[3], float radius, bool* effective) { // culling_system.cpp:225-242
	*effective = false;
	if (!pos) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null pos");
	uint32_t idx;
	const DV3 p = DV3{pos[0], pos[1], pos[2]};
	switch (locate(cs, entity, &idx)) {
		case Where::STATIC: {
			CullRec& r = cs.recs[idx];
			const IV3 c = cell_of(p);
			if (r.big == is_big_radius(radius) && c.x == r.cell.x && c.y == r.cell.y && c.z == r.cell.z) {
				r.radius = radius;
				r.rel = to_v3(sub(p, cell_origin(r.cell)));
				mark_patch(cs, idx);
			} else {
				readd_static(cs, idx, p, radius);
			}
			*effective = true;
			return LMX_OK;
		}
		case Where::DYNAMIC: {
			DynRec& r = cs.dyn[idx];
			if (r.bound && device_owns_bound) return LMX_OK; // lmx_world_propagate already refreshed this sphere on the device
			r.pos[0] = p.x; r.pos[1] = p.y; r.pos[2] = p.z;
			r.radius = radius;
			queue_dyn_patch(cs, r, true);
			*effective = true;
			return LMX_OK;
		}
		case Where::NONE: break;
	}
	return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %d is not in the culling system", entity);
}

static int cull_set_position_impl(LmxContext* ctx, CullSet& cs, bool device_owns_bound, bool replay, int32_t entity, const double pos[3], bool* effective) { // culling_system.cpp:201-217
	*effective = false;
	if (!pos) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null pos");
	uint32_t idx;
	const DV3 p = DV3{pos[0], pos[1], pos[2]};
	switch (locate(cs, entity, &idx)) {
		case Where::STATIC: {
			CullRec& r = cs.recs[idx];
			const IV3 c = cell_of(p);
			if (c.x == r.cell.x && c.y == r.cell.y && c.z == r.cell.z) {
				r.rel = to_v3(sub(p, cell_origin(r.cell)));
				mark_patch(cs, idx);
			} else {
				readd_static(cs, idx, p, r.radius);
			}
			*effective = true;
			return LMX_OK;
		}
		case Where::DYNAMIC: {
			if (cs.dyn[idx].bound) { // the radius the patch carries must be the one the device last computed
				if (device_owns_bound) return LMX_OK;
				if (!replay) { // (the shadow set's copy of a bound sphere is overwritten from the live device set when the sets trade places)
					if (int rc = cull_dyn_sync_mirror(ctx)) return rc;
				}
			}
			DynRec& r = cs.dyn[idx];
			r.pos[0] = p.x; r.pos[1] = p.y; r.pos[2] = p.z;
			queue_dyn_patch(cs, r, true);
			*effective = true;
			return LMX_OK;
		}
		case Where::NONE: break;
	}
	return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %d is not in the culling system", entity);
}

static int cull_set_radius_impl(LmxContext* ctx, CullSet& cs, bool device_owns_bound, bool replay, int32_t entity, float radius, bool* effective) { // culling_system.cpp:244-260
	*effective = false;
	uint32_t idx;
	switch (locate(cs, entity, &idx)) {
		case Where::STATIC: {
			CullRec& r = cs.recs[idx];
			if (r.big == is_big_radius(radius)) {
				r.radius = radius;
				mark_patch(cs, idx);
			} else {
				readd_static(cs, idx, add(cell_origin(r.cell), r.rel), radius); // pos = cell.header.origin + sphere->position
			}
			*effective = true;
			return LMX_OK;
		}
		case Where::DYNAMIC: {
			if (cs.dyn[idx].bound) {
				if (device_owns_bound) return LMX_OK;
				if (!replay) {
					if (int rc = cull_dyn_sync_mirror(ctx)) return rc;
				}
			}
			DynRec& r = cs.dyn[idx];
			if (is_big_radius(r.radius) != is_big_radius(radius)) {
				// the reference re-adds at origin + fp32 relative position, which loses the low bits of the position
				const DV3 p = stored_position(DV3{r.pos[0], r.pos[1], r.pos[2]});
				r.pos[0] = p.x; r.pos[1] = p.y; r.pos[2] = p.z;
			}
			r.radius = radius;
			queue_dyn_patch(cs, r, true);
			*effective = true;
			return LMX_OK;
		}
		case Where::NONE: break;
	}
	return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %d is not in the culling system", entity);
}


// lmx_world_bind_culling / unbind on a given set (see cull_make_dynamic)
static bool make_dynamic_impl(CullSet& cs, int32_t entity) {
	uint32_t idx;
	const Where w = locate(cs, entity, &idx);
	if (w == Where::DYNAMIC) {
		if (!cs.dyn[idx].bound) {
			cs.dyn[idx].bound = true;
			cs.n_unbound--;
		}
		return true;
	}
	if (w != Where::STATIC) return false;
	const CullRec r = cs.recs[idx];
	const DV3 pos = add(cell_origin(r.cell), r.rel);
	remove_static(cs, idx);
	dyn_append(cs, entity, r.type, pos, r.radius, true);
	return true;
}
static void unbind_impl(CullSet& cs, int32_t entity) {
	uint32_t idx;
	if (locate(cs, entity, &idx) == Where::DYNAMIC && cs.dyn[idx].bound) {
		cs.dyn[idx].bound = false;
		cs.n_unbound++;
	}
}

} // namespace

namespace lmx {

void queue_dyn_patch(CullSet& cs, const DynRec& r, bool alive) {
	if (r.slot == DYN_NO_SLOT || cs.dyn_layout_dirty) return; // the pending rebuild uploads the whole mirror
	const PatchDyn p{r.slot, alive ? r.entity : -1, r.radius, 0u, r.pos[0], r.pos[1], r.pos[2]};
	if (cs.q_dyn_at.size() < cs.dyn_padded) cs.q_dyn_at.resize(cs.dyn_padded, ~0u);
	uint32_t& at = cs.q_dyn_at[r.slot];
	if (at != ~0u) { // a freed slot taken again / an entity set twice before the next flush: the last write wins
		cs.q_dyn[at] = p;
		return;
	}
	at = (uint32_t)cs.q_dyn.size();
	cs.q_dyn.push_back(p);
}

// Move the unbound part of the dynamic set back into the static mirror (the next rebuild sorts it in).
void fold_overflow(CullSet& cs) {
	for (uint32_t i = (uint32_t)cs.dyn.size(); i-- > 0;) {
		if (cs.dyn[i].bound) continue;
		const DynRec r = cs.dyn[i];
		remove_dynamic(cs, i); // swaps the last record into i: already visited
		if ((size_t)r.entity >= cs.ent_to_rec.size()) cs.ent_to_rec.resize((size_t)r.entity + 1, -1);
		cs.ent_to_rec[r.entity] = (int32_t)cs.recs.size();
		cs.recs.push_back(make_cull_rec(r.entity, r.type, DV3{r.pos[0], r.pos[1], r.pos[2]}, r.radius));
	}
}

// The asynchronous compaction's replay of logged operations onto the shadow set (lmx_capi_cull_async.hip).
int async_replay(LmxContext* ctx, CullSet& cs, const CullOp* ops, size_t n) {
	for (size_t i = 0; i < n; ++i) {
		const CullOp& o = ops[i];
		bool eff;
		int rc = LMX_OK;
		switch (o.op) {
			case OP_ADD: rc = cull_add_impl(ctx, cs, o.entity, o.type, o.pos, o.radius); break;
			case OP_REMOVE: rc = cull_remove_impl(cs, o.entity, &eff); break;
			case OP_SET: rc = cull_set_impl(ctx, cs, false, o.entity, o.pos, o.radius, &eff); break;
			case OP_SET_POS: rc = cull_set_position_impl(ctx, cs, false, true, o.entity, o.pos, &eff); break;
			case OP_SET_RADIUS: rc = cull_set_radius_impl(ctx, cs, false, true, o.entity, o.radius, &eff); break;
			case OP_BIND: rc = make_dynamic_impl(cs, o.entity) ? LMX_OK : LMX_ERR_INVALID_ARGUMENT; break;
			case OP_UNBIND: unbind_impl(cs, o.entity); break;
			default: rc = LMX_ERR_INVALID_ARGUMENT;
		}
		if (rc != LMX_OK) return rc; // the shadow set has drifted from the live one: the job fails, the caller falls back to the synchronous path
	}
	return LMX_OK;
}

bool cull_make_dynamic(LmxContext* ctx, int32_t entity) {
	if (!make_dynamic_impl(ctx->cull, entity)) return false;
	async_log(ctx->cull, OP_BIND, entity, 0, nullptr, 0.f);
	return true;
}

void cull_unbind(LmxContext* ctx, int32_t entity) {
	unbind_impl(ctx->cull, entity);
	async_log(ctx->cull, OP_UNBIND, entity, 0, nullptr, 0.f);
}

} // namespace lmx

extern "C" {

// add / remove / set only touch the host mirror and the patch queues: no HIP call, no hipSetDevice per entity
int lmx_cull_add(LmxContext* ctx, int32_t entity, uint8_t type, const double pos[3], float radius) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	const int rc = cull_add_impl(ctx, ctx->cull, entity, type, pos, radius);
	if (rc == LMX_OK) async_log(ctx->cull, OP_ADD, entity, type, pos, radius);
	return rc;
}
int lmx_cull_remove(LmxContext* ctx, int32_t entity) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	bool effective;
	const int rc = cull_remove_impl(ctx->cull, entity, &effective);
	if (rc == LMX_OK && effective) async_log(ctx->cull, OP_REMOVE, entity, 0, nullptr, 0.f);
	return rc;
}
int lmx_cull_set(LmxContext* ctx, int32_t entity, const double pos[3], float radius) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	bool effective;
	const int rc = cull_set_impl(ctx, ctx->cull, ctx->cull.device_owns_bound, entity, pos, radius, &effective);
	if (rc == LMX_OK && effective) async_log(ctx->cull, OP_SET, entity, 0, pos, radius);
	return rc;
}

int lmx_cull_set_position(LmxContext* ctx, int32_t entity, const double pos[3]) { // culling_system.cpp:201-217
	LMX_CHECK_CTX(ctx);
	bool effective;
	const int rc = cull_set_position_impl(ctx, ctx->cull, ctx->cull.device_owns_bound, false, entity, pos, &effective);
	if (rc == LMX_OK && effective) async_log(ctx->cull, OP_SET_POS, entity, 0, pos, 0.f);
	return rc;
}

int lmx_cull_set_radius(LmxContext* ctx, int32_t entity, float radius) { // culling_system.cpp:244-260
	LMX_CHECK_CTX(ctx);
	bool effective;
	const int rc = cull_set_radius_impl(ctx, ctx->cull, ctx->cull.device_owns_bound, false, entity, radius, &effective);
	if (rc == LMX_OK && effective) async_log(ctx->cull, OP_SET_RADIUS, entity, 0, nullptr, radius);
	return rc;
}

int lmx_cull_get_radius(LmxContext* ctx, int32_t entity, float* out_radius) {
	LMX_CHECK_CTX(ctx);
	CullState& cs = ctx->cull;
	uint32_t idx;
	switch (locate(cs, entity, &idx)) {
		case Where::STATIC:
			if (out_radius) *out_radius = cs.recs[idx].radius;
			return LMX_OK;
		case Where::DYNAMIC:
			if (cs.dyn[idx].bound) {
				if (int rc = cull_dyn_sync_mirror(ctx)) return rc;
			}
			if (out_radius) *out_radius = cs.dyn[idx].radius;
			return LMX_OK;
		case Where::NONE: break;
	}
	return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %d is not in the culling system", entity);
}

int lmx_cull_is_added(LmxContext* ctx, int32_t entity) {
	if (!ctx) return 0;
	uint32_t idx;
	return locate(ctx->cull, entity, &idx) != Where::NONE ? 1 : 0;
}

// Batched forms of add / remove / set for hosts that pay per call (ctypes, scripting): same semantics, one ABI crossing. An update
// touches 3-5 random entries of tables that hold one element per entity (entity -> record, record, record -> device slot): with 10 M
// entities every one of them is a DRAM miss, and the misses of ONE update depend on each other. The batch forms run a two-stage
// software prefetch ahead of the update loop (entity -> record index PF_FAR updates ahead, the record and its slot PF_NEAR ahead), so
// the misses of neighbouring updates overlap.
constexpr uint32_t PF_FAR = 24, PF_NEAR = 12;
static inline void prefetch_update(const CullSet& cs, const int32_t* entity, uint32_t n, uint32_t i) {
	if (i + PF_FAR < n) {
		const int32_t e = entity[i + PF_FAR];
		if (e >= 0) {
			if ((size_t)e < cs.ent_to_rec.size()) __builtin_prefetch(&cs.ent_to_rec[e]);
			if ((size_t)e < cs.ent_to_dyn.size()) __builtin_prefetch(&cs.ent_to_dyn[e]);
		}
	}
	if (i + PF_NEAR < n) {
		const int32_t e = entity[i + PF_NEAR];
		if (e >= 0 && (size_t)e < cs.ent_to_rec.size()) {
			const int32_t r = cs.ent_to_rec[e]; // prefetched PF_FAR - PF_NEAR updates ago; may be stale by the time it is used: a hint only
			if (r >= 0 && (size_t)r < cs.recs.size()) {
				__builtin_prefetch(&cs.recs[r]);
				if ((size_t)r < cs.rec_slot.size()) __builtin_prefetch(&cs.rec_slot[r]);
			}
		}
		if (e >= 0 && (size_t)e < cs.ent_to_dyn.size()) {
			const int32_t d = cs.ent_to_dyn[e];
			if (d >= 0 && (size_t)d < cs.dyn.size()) __builtin_prefetch(&cs.dyn[d]);
		}
	}
}

int lmx_cull_add_many(LmxContext* ctx, uint32_t n, const int32_t* entity, const uint8_t* type, const double* pos_xyz, const float* radius) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	if (n && (!entity || !type || !pos_xyz || !radius)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null input array");
	for (uint32_t i = 0; i < n; ++i) {
		prefetch_update(ctx->cull, entity, n, i);
		if (int rc = cull_add_impl(ctx, ctx->cull, entity[i], type[i], pos_xyz + 3 * (size_t)i, radius[i])) return rc;
		async_log(ctx->cull, OP_ADD, entity[i], type[i], pos_xyz + 3 * (size_t)i, radius[i]);
	}
	return LMX_OK;
}

int lmx_cull_set_many(LmxContext* ctx, uint32_t n, const int32_t* entity, const double* pos_xyz, const float* radius) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	if (n && (!entity || !pos_xyz || !radius)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null input array");
	for (uint32_t i = 0; i < n; ++i) {
		prefetch_update(ctx->cull, entity, n, i);
		bool effective;
		if (int rc = cull_set_impl(ctx, ctx->cull, ctx->cull.device_owns_bound, entity[i], pos_xyz + 3 * (size_t)i, radius[i], &effective)) return rc;
		if (effective) async_log(ctx->cull, OP_SET, entity[i], 0, pos_xyz + 3 * (size_t)i, radius[i]);
	}
	return LMX_OK;
}

int lmx_cull_remove_many(LmxContext* ctx, uint32_t n, const int32_t* entity) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	if (n && !entity) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null input array");
	for (uint32_t i = 0; i < n; ++i) {
		prefetch_update(ctx->cull, entity, n, i);
		bool effective;
		if (int rc = cull_remove_impl(ctx->cull, entity[i], &effective)) return rc;
		if (effective) async_log(ctx->cull, OP_REMOVE, entity[i], 0, nullptr, 0.f);
	}
	return LMX_OK;
}

} // extern "C"
