// world_edit_kernels.hip — structural edits of the world mirror on gfx950: World::destroyEntity / createEntity / setParent
// (src/engine/world.cpp:521-561, 489-519, 619-701) for a batch, without the transforms leaving HBM.
//
// The slot order is the one lmx_capi_world.hip's world_rebuild defines - levels, within a level by parent slot, siblings and roots by
// entity index - derived here from the edited `parent` array: a stable sort of (parent + 1, entity) groups the children of every parent
// in entity order behind the roots, and the levels are expanded one by one from the roots (children per slot, exclusive sum, scatter).
// Dead entities are childless roots. Nothing below takes a place from an atomic: two runs give identical bytes.
#include "lmx_kernels.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

constexpr uint32_t EDIT_NONE = 0xffffffffu;

__global__ __launch_bounds__(256) void k_edit_mark(uint8_t* __restrict__ mark, const int32_t* __restrict__ list, uint32_t n) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n) mark[list[i]] = 1; // (a duplicate writes the same byte)
}

// destroyEntity takes the subtree with it: an entity dies when it or one of its ancestors - by the parents of BEFORE the call - is listed
__global__ __launch_bounds__(256) void k_edit_kill(const int32_t* __restrict__ parent, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ mark,
	uint8_t* __restrict__ kill, uint32_t n) {
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= n) return;
	uint8_t k = 0;
	if (alive[e])
		for (int32_t a = (int32_t)e; a >= 0; a = parent[a])
			if (mark[a]) { k = 1; break; }
	kill[e] = k;
}

__global__ __launch_bounds__(256) void k_edit_bury(int32_t* __restrict__ parent, uint8_t* __restrict__ alive, const uint8_t* __restrict__ kill, uint32_t n) {
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= n || !kill[e]) return;
	alive[e] = 0;
	parent[e] = -1;
}

// created entities come alive as roots (a dead entity's parent is -1 already); every re-parented child gets its last parent of the list
__global__ __launch_bounds__(256) void k_edit_link(int32_t* __restrict__ parent, uint8_t* __restrict__ alive, const int32_t* __restrict__ create, uint32_t n_create,
	const int32_t* __restrict__ child, const int32_t* __restrict__ new_parent, uint32_t n_reparent) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n_create) alive[create[i]] = 1;
	if (i < n_reparent) parent[child[i]] = new_parent[i] < 0 ? -1 : new_parent[i];
}

// the sort's pairs, and the number of live entities: one add per block of a capped grid (a sum does not depend on the order of its terms;
// an add per wave of 10^6 entities is 15.6 k atomics on one address, 180 us - the whole pass otherwise takes 10)
constexpr uint32_t EDIT_KEYS_MAX_BLOCKS = 1024;
__global__ __launch_bounds__(256) void k_edit_keys(const int32_t* __restrict__ parent, const uint8_t* __restrict__ alive, uint32_t n, uint32_t* __restrict__ key,
	uint32_t* __restrict__ value, uint32_t* __restrict__ n_live) {
	__shared__ uint32_t s_wave[4];
	uint32_t mine = 0;
	for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) { // block-uniform trip count
		const uint32_t e = base + threadIdx.x;
		if (e < n) {
			key[e] = (uint32_t)(parent[e] + 1);
			value[e] = e;
			mine += alive[e] != 0 ? 1u : 0u;
		}
	}
	uint32_t total;
	const uint32_t upto = block_scan<false>(mine, 4u, 0u, s_wave, &total, Sum()); // inclusive: the last thread holds the block's sum
	if (threadIdx.x == 255u && upto) atomicAdd(n_live, upto);
}

// sorted keys -> where the children of parent p stand in the sorted list: [first[p + 1], first[p + 1] + count[p + 1]); [0] are the roots
__global__ __launch_bounds__(256) void k_edit_child_ranges(const uint32_t* __restrict__ key, uint32_t n, uint32_t* __restrict__ first, uint32_t* __restrict__ count) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t k = key[i];
	if (i == 0 || key[i - 1] != k) first[k] = i;
	if (i + 1 == n || key[i + 1] != k) count[k] = i + 1; // the range's end for now: k_edit_child_counts takes the start off
}
__global__ __launch_bounds__(256) void k_edit_child_counts(const uint32_t* __restrict__ first, uint32_t* __restrict__ count, uint32_t n) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k < n && count[k]) count[k] -= first[k];
}

struct EditOrder {
	const uint32_t* sorted;  // entities grouped by parent
	const uint32_t* first;   // [n + 1]
	const uint32_t* count;   // [n + 1]
	int32_t* entity_of_slot; // the new order
	int32_t* slot_of_entity;
	int32_t* parent_slot;
	uint32_t* root_of_slot;  // the level-0 slot every slot hangs under (the run table's cut)
};

__global__ __launch_bounds__(256) void k_edit_roots(EditOrder o, uint32_t n_roots) {
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s >= n_roots) return;
	const uint32_t e = o.sorted[s];
	o.entity_of_slot[s] = (int32_t)e;
	o.slot_of_entity[e] = (int32_t)s;
	o.parent_slot[s] = -1;
	o.root_of_slot[s] = s;
}

__device__ __forceinline__ void edit_place_children(const EditOrder& o, uint32_t parent_slot, uint32_t e, uint32_t n_children, uint32_t at) {
	const uint32_t c0 = o.first[e + 1];
	const uint32_t root = o.root_of_slot[parent_slot];
	for (uint32_t k = 0; k < n_children; ++k) {
		const uint32_t c = o.sorted[c0 + k];
		o.entity_of_slot[at + k] = (int32_t)c;
		o.slot_of_entity[c] = (int32_t)(at + k);
		o.parent_slot[at + k] = (int32_t)parent_slot;
		o.root_of_slot[at + k] = root;
	}
}

// one level of at most 256 slots: counts, the block's exclusive sum and the scatter in one launch; *total = the next level's size
__global__ __launch_bounds__(256) void k_edit_level_small(EditOrder o, uint32_t level_first, uint32_t m, uint32_t* __restrict__ total) {
	__shared__ uint32_t s_wave[4];
	const uint32_t tid = threadIdx.x;
	const uint32_t e = tid < m ? (uint32_t)o.entity_of_slot[level_first + tid] : 0u;
	const uint32_t c = tid < m ? o.count[e + 1] : 0u;
	uint32_t all;
	const uint32_t at = block_scan<true>(c, 4u, 0u, s_wave, &all, Sum());
	if (tid < m) edit_place_children(o, level_first + tid, e, c, level_first + m + at);
	if (tid == 255u) *total = at + c; // (= all: the last thread's exclusive prefix and its own count)
}

// a wider level in three steps: counts (one more word, zero, so that the sum's last word is the total), hipcub's sum, scatter
__global__ __launch_bounds__(256) void k_edit_level_count(EditOrder o, uint32_t level_first, uint32_t m, uint32_t* __restrict__ cnt) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i > m) return;
	cnt[i] = i < m ? o.count[(uint32_t)o.entity_of_slot[level_first + i] + 1u] : 0u;
}
__global__ __launch_bounds__(256) void k_edit_level_scatter(EditOrder o, uint32_t level_first, uint32_t m, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= m) return;
	edit_place_children(o, level_first + i, (uint32_t)o.entity_of_slot[level_first + i], cnt[i], level_first + m + off[i]);
}

// old slot -> new slot for the 14 arrays and the per-slot culling tables; an index without an old slot (grown range) reads as zero
__global__ __launch_bounds__(256) void k_edit_permute(WorldDevice from, WorldDevice to, const int32_t* __restrict__ entity_of_slot, const int32_t* __restrict__ old_slot_of_entity,
	const uint8_t* __restrict__ kill, uint32_t n_old, uint32_t n, const uint32_t* __restrict__ dyn_from, const float* __restrict__ radius_from, uint32_t* __restrict__ dyn_to,
	float* __restrict__ radius_to) {
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s >= n) return;
	const uint32_t e = (uint32_t)entity_of_slot[s];
	if (e < n_old) {
		const int32_t o = old_slot_of_entity[e];
		to.lpx[s] = from.lpx[o]; to.lpy[s] = from.lpy[o]; to.lpz[s] = from.lpz[o]; to.lrot[s] = from.lrot[o];
		to.lsx[s] = from.lsx[o]; to.lsy[s] = from.lsy[o]; to.lsz[s] = from.lsz[o];
		to.wpx[s] = from.wpx[o]; to.wpy[s] = from.wpy[o]; to.wpz[s] = from.wpz[o]; to.wrot[s] = from.wrot[o];
		to.wsx[s] = from.wsx[o]; to.wsy[s] = from.wsy[o]; to.wsz[s] = from.wsz[o];
		if (dyn_to != nullptr) {
			const bool keep = kill[e] == 0; // a destroyed entity's binding is dropped, also when the index was created again
			dyn_to[s] = keep ? dyn_from[o] : EDIT_NONE;
			radius_to[s] = keep ? radius_from[o] : 0.f;
		}
	} else {
		const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
		to.lpx[s] = 0.0; to.lpy[s] = 0.0; to.lpz[s] = 0.0; to.lrot[s] = z; to.lsx[s] = 0.f; to.lsy[s] = 0.f; to.lsz[s] = 0.f;
		to.wpx[s] = 0.0; to.wpy[s] = 0.0; to.wpz[s] = 0.0; to.wrot[s] = z; to.wsx[s] = 0.f; to.wsy[s] = 0.f; to.wsz[s] = 0.f;
		if (dyn_to != nullptr) {
			dyn_to[s] = EDIT_NONE;
			radius_to[s] = 0.f;
		}
	}
}

struct EditTransformAoS { double pos[3]; float rot[4]; float scale[3]; float pad; }; // LmxTransform, 56 B

__global__ __launch_bounds__(256) void k_edit_create(WorldDevice w, const int32_t* __restrict__ slot_of_entity, const int32_t* __restrict__ create,
	const EditTransformAoS* __restrict__ tr, uint32_t n) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const int32_t s = slot_of_entity[create[i]];
	const EditTransformAoS t = tr[i];
	w.wpx[s] = t.pos[0]; w.wpy[s] = t.pos[1]; w.wpz[s] = t.pos[2];
	w.wrot[s] = make_float4(t.rot[0], t.rot[1], t.rot[2], t.rot[3]);
	w.wsx[s] = t.scale[0]; w.wsy[s] = t.scale[1]; w.wsz[s] = t.scale[2];
}

// World::setParent's local (world.cpp:660-664): Transform::computeLocal(parent world, child world). World values do not change in an
// edit, so every child of the list reads final values whatever the list's order was.
__global__ __launch_bounds__(256) void k_edit_locals(WorldDevice w, const int32_t* __restrict__ slot_of_entity, const int32_t* __restrict__ child,
	const int32_t* __restrict__ new_parent, uint32_t n) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n || new_parent[i] < 0) return;
	const int32_t s = slot_of_entity[child[i]], p = slot_of_entity[new_parent[i]];
	Xform parent, me;
	const float4 pr = w.wrot[p], mr = w.wrot[s];
	parent.pos = DV3{w.wpx[p], w.wpy[p], w.wpz[p]};
	parent.rot = Q4{pr.x, pr.y, pr.z, pr.w};
	parent.scale = V3{w.wsx[p], w.wsy[p], w.wsz[p]};
	me.pos = DV3{w.wpx[s], w.wpy[s], w.wpz[s]};
	me.rot = Q4{mr.x, mr.y, mr.z, mr.w};
	me.scale = V3{w.wsx[s], w.wsy[s], w.wsz[s]};
	const Xform l = compute_local(parent, me);
	w.lpx[s] = l.pos.x; w.lpy[s] = l.pos.y; w.lpz[s] = l.pos.z;
	w.lrot[s] = make_float4(l.rot.x, l.rot.y, l.rot.z, l.rot.w);
	w.lsx[s] = l.scale.x; w.lsy[s] = l.scale.y; w.lsz[s] = l.scale.z;
}

__device__ __forceinline__ uint32_t edit_new_slot(uint32_t old_slot, const int32_t* old_entity_of_slot, const int32_t* slot_of_entity, const uint8_t* kill) {
	if (old_slot == EDIT_NONE) return EDIT_NONE;
	const int32_t e = old_entity_of_slot[old_slot];
	return kill[e] ? EDIT_NONE : (uint32_t)slot_of_entity[e];
}

// the records that name slots: the culling binding's list and the bone attachments. One whose entity (or attachment parent) died is void.
__global__ __launch_bounds__(256) void k_edit_remap(const int32_t* __restrict__ old_entity_of_slot, const int32_t* __restrict__ slot_of_entity, const uint8_t* __restrict__ kill,
	uint32_t* __restrict__ bound_slot, uint32_t n_bound, BoneAttachDevice* __restrict__ attach, uint32_t n_attach) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n_bound) bound_slot[i] = edit_new_slot(bound_slot[i], old_entity_of_slot, slot_of_entity, kill);
	if (i < n_attach) {
		const uint32_t s = edit_new_slot(attach[i].slot, old_entity_of_slot, slot_of_entity, kill);
		const uint32_t p = attach[i].slot == EDIT_NONE ? EDIT_NONE : edit_new_slot(attach[i].parent_slot, old_entity_of_slot, slot_of_entity, kill);
		attach[i].slot = p == EDIT_NONE ? EDIT_NONE : s;
		attach[i].parent_slot = s == EDIT_NONE ? EDIT_NONE : p;
	}
}

// the bindings this call voids, for the host's list: entry i of the binding list whose entity dies. The host only marks them, so the
// order they arrive in here reaches nothing.
__global__ __launch_bounds__(256) void k_edit_dropped(const int32_t* __restrict__ old_entity_of_slot, const uint8_t* __restrict__ kill, const uint32_t* __restrict__ bound_slot,
	uint32_t n_bound, uint32_t* __restrict__ dropped, uint32_t* __restrict__ count) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const uint32_t o = i < n_bound ? bound_slot[i] : EDIT_NONE;
	const bool dies = o != EDIT_NONE && kill[old_entity_of_slot[o]] != 0;
	const uint32_t at = wave_append(dies, count);
	if (dies) dropped[at] = i; // (at < n_bound: every entry is appended once at the most)
}

// first slot of level [first, end) whose root is `r` or a later one: a level is ordered by root
__device__ __forceinline__ uint32_t edit_lower_bound(const uint32_t* __restrict__ root_of_slot, uint32_t first, uint32_t end, uint32_t r) {
	while (first < end) {
		const uint32_t mid = first + ((end - first) >> 1);
		if (root_of_slot[mid] < r) first = mid + 1u;
		else end = mid;
	}
	return first;
}

__global__ __launch_bounds__(256) void k_edit_root_sizes(const uint32_t* __restrict__ root_of_slot, const uint32_t* __restrict__ level_start, uint32_t n_levels, uint32_t n_roots,
	uint32_t* __restrict__ size) {
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n_roots) return;
	uint32_t sum = 1;
	for (uint32_t l = 1; l < n_levels; ++l) {
		const uint32_t a = edit_lower_bound(root_of_slot, level_start[l], level_start[l + 1], r);
		sum += edit_lower_bound(root_of_slot, a, level_start[l + 1], r + 1u) - a;
	}
	size[r] = sum;
}

// k_xform_subtree's table: row i = per level the first slot of the run that begins with root run_root[i] (the last row: n_roots)
__global__ __launch_bounds__(256) void k_edit_run_table(const uint32_t* __restrict__ root_of_slot, const uint32_t* __restrict__ level_start, uint32_t n_levels,
	const uint32_t* __restrict__ run_root, uint32_t n_rows, uint32_t* __restrict__ table) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n_rows * n_levels) return;
	const uint32_t row = i / n_levels, l = i % n_levels;
	table[i] = l == 0 ? run_root[row] : edit_lower_bound(root_of_slot, level_start[l], level_start[l + 1], run_root[row]);
}

inline dim3 edit_grid(uint32_t n) { return dim3((n + 255u) / 256u); }

} // namespace

hipError_t launch_edit_kill(hipStream_t s, const WorldEditDevice& d, const int32_t* destroy, uint32_t n_destroy, uint32_t n_old) {
	if (!n_destroy || !n_old) return hipSuccess;
	hipLaunchKernelGGL(k_edit_mark, edit_grid(n_destroy), dim3(256), 0, s, d.mark, destroy, n_destroy);
	hipLaunchKernelGGL(k_edit_kill, edit_grid(n_old), dim3(256), 0, s, d.parent, d.alive, d.mark, d.kill, n_old);
	hipLaunchKernelGGL(k_edit_bury, edit_grid(n_old), dim3(256), 0, s, d.parent, d.alive, d.kill, n_old);
	return hipGetLastError();
}

hipError_t launch_edit_link(hipStream_t s, const WorldEditDevice& d, const int32_t* create, uint32_t n_create, const int32_t* child, const int32_t* new_parent, uint32_t n_reparent) {
	const uint32_t n = n_create > n_reparent ? n_create : n_reparent;
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_edit_link, edit_grid(n), dim3(256), 0, s, d.parent, d.alive, create, n_create, child, new_parent, n_reparent);
	return hipGetLastError();
}

hipError_t launch_edit_keys(hipStream_t s, const WorldEditDevice& d, uint32_t n, uint32_t* key, uint32_t* value, uint32_t* n_live) {
	if (!n) return hipSuccess;
	const uint32_t blocks = (n + 255u) / 256u;
	hipLaunchKernelGGL(k_edit_keys, dim3(blocks < EDIT_KEYS_MAX_BLOCKS ? blocks : EDIT_KEYS_MAX_BLOCKS), dim3(256), 0, s, d.parent, d.alive, n, key, value, n_live);
	return hipGetLastError();
}

hipError_t launch_edit_child_ranges(hipStream_t s, const uint32_t* sorted_key, uint32_t n, uint32_t* first, uint32_t* count) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_edit_child_ranges, edit_grid(n), dim3(256), 0, s, sorted_key, n, first, count);
	hipLaunchKernelGGL(k_edit_child_counts, edit_grid(n + 1u), dim3(256), 0, s, first, count, n + 1u);
	return hipGetLastError();
}

static EditOrder edit_order(const WorldEditOrder& o) {
	EditOrder k;
	k.sorted = o.sorted; k.first = o.first; k.count = o.count; k.entity_of_slot = o.entity_of_slot; k.slot_of_entity = o.slot_of_entity;
	k.parent_slot = o.parent_slot; k.root_of_slot = o.root_of_slot;
	return k;
}

hipError_t launch_edit_roots(hipStream_t s, const WorldEditOrder& o, uint32_t n_roots) {
	if (!n_roots) return hipSuccess;
	hipLaunchKernelGGL(k_edit_roots, edit_grid(n_roots), dim3(256), 0, s, edit_order(o), n_roots);
	return hipGetLastError();
}

hipError_t launch_edit_level_small(hipStream_t s, const WorldEditOrder& o, uint32_t level_first, uint32_t m, uint32_t* total) {
	if (!m || m > WORLD_EDIT_SMALL_LEVEL) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_edit_level_small, dim3(1), dim3(256), 0, s, edit_order(o), level_first, m, total);
	return hipGetLastError();
}

hipError_t launch_edit_level_count(hipStream_t s, const WorldEditOrder& o, uint32_t level_first, uint32_t m, uint32_t* cnt) {
	hipLaunchKernelGGL(k_edit_level_count, edit_grid(m + 1u), dim3(256), 0, s, edit_order(o), level_first, m, cnt);
	return hipGetLastError();
}

hipError_t launch_edit_level_scatter(hipStream_t s, const WorldEditOrder& o, uint32_t level_first, uint32_t m, const uint32_t* cnt, const uint32_t* off) {
	if (!m) return hipSuccess;
	hipLaunchKernelGGL(k_edit_level_scatter, edit_grid(m), dim3(256), 0, s, edit_order(o), level_first, m, cnt, off);
	return hipGetLastError();
}

hipError_t launch_edit_permute(hipStream_t s, const WorldDevice& from, const WorldDevice& to, const int32_t* entity_of_slot, const int32_t* old_slot_of_entity, const uint8_t* kill,
	uint32_t n_old, uint32_t n, const uint32_t* dyn_from, const float* radius_from, uint32_t* dyn_to, float* radius_to) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_edit_permute, edit_grid(n), dim3(256), 0, s, from, to, entity_of_slot, old_slot_of_entity, kill, n_old, n, dyn_from, radius_from, dyn_to, radius_to);
	return hipGetLastError();
}

hipError_t launch_edit_create(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const int32_t* create, const void* transforms, uint32_t n) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_edit_create, edit_grid(n), dim3(256), 0, s, w, slot_of_entity, create, (const EditTransformAoS*)transforms, n);
	return hipGetLastError();
}

hipError_t launch_edit_locals(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const int32_t* child, const int32_t* new_parent, uint32_t n) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_edit_locals, edit_grid(n), dim3(256), 0, s, w, slot_of_entity, child, new_parent, n);
	return hipGetLastError();
}

hipError_t launch_edit_remap(hipStream_t s, const int32_t* old_entity_of_slot, const int32_t* slot_of_entity, const uint8_t* kill, uint32_t* bound_slot, uint32_t n_bound,
	BoneAttachDevice* attach, uint32_t n_attach) {
	const uint32_t n = n_bound > n_attach ? n_bound : n_attach;
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_edit_remap, edit_grid(n), dim3(256), 0, s, old_entity_of_slot, slot_of_entity, kill, bound_slot, n_bound, attach, n_attach);
	return hipGetLastError();
}

hipError_t launch_edit_dropped(hipStream_t s, const int32_t* old_entity_of_slot, const uint8_t* kill, const uint32_t* bound_slot, uint32_t n_bound, uint32_t* dropped,
	uint32_t* count) {
	if (!n_bound) return hipSuccess;
	hipLaunchKernelGGL(k_edit_dropped, edit_grid(n_bound), dim3(256), 0, s, old_entity_of_slot, kill, bound_slot, n_bound, dropped, count);
	return hipGetLastError();
}

hipError_t launch_edit_root_sizes(hipStream_t s, const uint32_t* root_of_slot, const uint32_t* level_start, uint32_t n_levels, uint32_t n_roots, uint32_t* size) {
	if (!n_roots) return hipSuccess;
	hipLaunchKernelGGL(k_edit_root_sizes, edit_grid(n_roots), dim3(256), 0, s, root_of_slot, level_start, n_levels, n_roots, size);
	return hipGetLastError();
}

hipError_t launch_edit_run_table(hipStream_t s, const uint32_t* root_of_slot, const uint32_t* level_start, uint32_t n_levels, const uint32_t* run_root, uint32_t n_rows,
	uint32_t* table) {
	if (!n_rows || !n_levels) return hipSuccess;
	hipLaunchKernelGGL(k_edit_run_table, edit_grid(n_rows * n_levels), dim3(256), 0, s, root_of_slot, level_start, n_levels, run_root, n_rows, table);
	return hipGetLastError();
}

} // namespace lmx
