// draw_kernels.hip — PipelineImpl::createCommands (renderer/pipeline.cpp:2747-3320) and the "fill instance data" block of createSortKeys
// (:3970-4014) on the device: the sorted (key, value) pairs are cut into runs (one draw call each) and every pair gets its instance record,
// byte for byte as the reference's memcpy / struct stores write it. FMA-free (-ffp-contract=off); the fp64 subtract + convert of
// Vec3(tr.pos - camera_pos) is the only fp64 work.
//
// The reference's walk is sequential per batch (:2810): a head picks its rule (unmoved MESH: while the MASKED key is equal, :3094-3097; moved MESH,
// SKINNED, DECAL, CURVE_DECAL: while the FULL key is equal; AUTOINSTANCED: one pair) and the next head is wherever that run ends. It is
// not loop-carried: with M = masked-key break (or batch start), F = full-key break (M implies F), A = "a head here takes one pair",
// U = unmoved MESH, a two-bit state {streak, blocked} walks the pairs
//     M: blocked = 0;  F: streak = 1;  head = streak && !blocked;  then, if streak && !A: { blocked |= U; streak = 0 }
// (streak: every pair of this full-key segment so far was a one-pair head; blocked: an unmoved MESH head swallows the rest of the masked
// segment). A pair's step is a function {0..3} -> {0..3}: eight bits, composed associatively - a scan (wave shuffles, the waves of a
// block through LDS, the blocks through one small launch), no thread per batch.
#include "lmx_kernels.h"
#include "lmx_entity_tr.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

enum { DRAW_F_M = 1, DRAW_F_F = 2, DRAW_F_A = 4, DRAW_F_U = 8 };
constexpr uint32_t FN_IDENTITY = 0xE4u; // s -> s for s = 0..3, two bits each

__device__ __forceinline__ uint32_t fn_of_flags(uint32_t fl) {
	uint32_t f = 0;
	for (uint32_t s = 0; s < 4; ++s) {
		uint32_t streak = s & 1u, blocked = s >> 1;
		if (fl & DRAW_F_M) blocked = 0;
		if (fl & DRAW_F_F) streak = 1;
		if (streak && !(fl & DRAW_F_A)) {
			if (fl & DRAW_F_U) blocked = 1;
			streak = 0;
		}
		f |= (streak | (blocked << 1)) << (2 * s);
	}
	return f;
}
__device__ __forceinline__ uint32_t fn_apply(uint32_t f, uint32_t s) { return (f >> (2 * s)) & 3u; }
// first f, then g
__device__ __forceinline__ uint32_t fn_compose(uint32_t f, uint32_t g) {
	return fn_apply(g, fn_apply(f, 0)) | (fn_apply(g, fn_apply(f, 1)) << 2) | (fn_apply(g, fn_apply(f, 2)) << 4) | (fn_apply(g, fn_apply(f, 3)) << 6);
}
__device__ __forceinline__ bool head_of(uint32_t fl, uint32_t state_before) {
	uint32_t streak = state_before & 1u, blocked = state_before >> 1;
	if (fl & DRAW_F_M) blocked = 0;
	if (fl & DRAW_F_F) streak = 1;
	return streak && !blocked;
}

// Inclusive scan of the block's functions in thread order; *total = the block's composition. s_wave: one word per wave.
struct FnCompose {
	__device__ __forceinline__ uint32_t operator()(uint32_t f, uint32_t g) const { return fn_compose(f, g); }
};
__device__ __forceinline__ uint32_t block_scan_fn(uint32_t f, uint32_t* s_wave, uint32_t* total) {
	return block_scan<false>(f, blockDim.x >> 6, FN_IDENTITY, s_wave, total, FnCompose());
}

__device__ __forceinline__ uint64_t key_mask(const DrawViewDevice& v, uint64_t key) { // instance_key_mask, :2824-2825
	const uint32_t b = (uint32_t)(key >> LMX_SORT_KEY_BUCKET_SHIFT);
	return (v.depth_sorted[b >> 5] >> (b & 31u)) & 1u ? 0xff00000000ffffffull : 0xffffffff00000000ull;
}
__device__ __forceinline__ uint32_t type_of(uint64_t value) { return (uint32_t)(value >> LMX_SORT_VALUE_TYPE_SHIFT) & 31u; } // SORT_VALUE_TYPE_MASK, :75
__device__ __forceinline__ bool entity_moved(const DrawDevice& d, uint32_t e) {
	return e < d.n_entities && (d.inst[e].flags & LMX_MODEL_INSTANCE_MOVED) != 0;
}

// Pass 1: one pair per lane: its flags, and the composition of its tile.
__global__ __launch_bounds__(DRAW_TILE) void k_draw_flags(DrawDevice d, DrawViewDevice v) {
	__shared__ uint32_t s_wave[DRAW_TILE / 64];
	const uint32_t i = blockIdx.x * DRAW_TILE + threadIdx.x;
	uint32_t fl = 0;
	if (i < d.n) {
		const uint64_t key = d.keys[i], value = d.values[i];
		const uint32_t type = type_of(value);
		if (i % d.step == 0) {
			fl = DRAW_F_M | DRAW_F_F;
		} else {
			const uint64_t prev = d.keys[i - 1];
			const uint64_t mask = key_mask(v, key);
			if (prev != key) fl |= DRAW_F_F;
			if ((prev & mask) != (key & mask)) fl |= DRAW_F_M;
		}
		if (type == LMX_DRAW_AUTOINSTANCED || type > LMX_DRAW_CURVE_DECAL) fl |= DRAW_F_A;
		if (type == LMX_DRAW_MESH && !entity_moved(d, (uint32_t)value)) fl |= DRAW_F_U;
		d.flags[i] = (uint8_t)fl;
	}
	uint32_t total;
	(void)block_scan_fn(i < d.n ? fn_of_flags(fl) : FN_IDENTITY, s_wave, &total);
	if (threadIdx.x == 0) d.tile_fn[blockIdx.x] = (uint8_t)total;
}

// Pass 2 (one block, DRAW_TILE tiles per round with a carry): the state behind every tile.
__global__ __launch_bounds__(DRAW_TILE) void k_draw_tile_scan(DrawDevice d, uint32_t n_tiles) {
	__shared__ uint32_t s_wave[DRAW_TILE / 64];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += DRAW_TILE) {
		const uint32_t t = base + threadIdx.x;
		const uint32_t f = t < n_tiles ? d.tile_fn[t] : FN_IDENTITY;
		uint32_t total;
		const uint32_t incl = block_scan_fn(f, s_wave, &total);
		if (t < n_tiles) d.tile_in[t] = (uint8_t)fn_apply(incl, carry); // the state BEHIND tile t: tile t + 1 starts from it (k_draw_heads)
		carry = fn_apply(total, carry);
	}
}

// Pass 3: head flags.
__global__ __launch_bounds__(DRAW_TILE) void k_draw_heads(DrawDevice d) {
	__shared__ uint32_t s_wave[DRAW_TILE / 64];
	__shared__ uint32_t s_incl[DRAW_TILE];
	const uint32_t i = blockIdx.x * DRAW_TILE + threadIdx.x;
	const uint32_t fl = i < d.n ? d.flags[i] : 0u;
	uint32_t total;
	s_incl[threadIdx.x] = block_scan_fn(i < d.n ? fn_of_flags(fl) : FN_IDENTITY, s_wave, &total);
	__syncthreads();
	const uint32_t tile_state = blockIdx.x ? d.tile_in[blockIdx.x - 1] : 0u; // tile_in[t] holds the state behind tile t
	const uint32_t before = threadIdx.x ? fn_apply(s_incl[threadIdx.x - 1], tile_state) : tile_state;
	if (i < d.n) d.head[i] = head_of(fl, before) ? 1u : 0u;
	if (i == d.n) d.head[i] = 0;
}

// DrawTr / load_tr(d, e) - transforms[e], uploaded or the propagated world in place - are shared with the cluster pass: lmx_entity_tr.h
__device__ __forceinline__ uint32_t rel_bits(double p, double cam) { return __float_as_uint((float)(p - cam)); } // Vec3(tr.pos - camera_pos), one component

// Mesh::lod of mesh `mesh_idx` of entity e's model (0 where the entity has no such mesh)
__device__ __forceinline__ float mesh_lod_of(const DrawDevice& d, uint32_t e, uint32_t mesh_idx) {
	if (e >= d.n_entities) return 0.0f;
	const int32_t m = d.inst[e].model;
	if (m < 0 || (uint32_t)m >= d.n_models) return 0.0f;
	const LmxKeysModel& md = d.models[m];
	if (mesh_idx >= md.mesh_count || md.first_mesh + mesh_idx >= d.n_meshes) return 0.0f;
	return d.mesh_lod[md.first_mesh + mesh_idx];
}
// model_instances[e].mesh_materials[mesh_idx].material_index
__device__ __forceinline__ uint32_t material_of(const DrawDevice& d, uint32_t e, uint32_t mesh_idx) {
	if (e >= d.n_entities) return 0;
	const KeysInstance& r = d.inst[e];
	if (r.model < 0 || (uint32_t)r.model >= d.n_models || mesh_idx >= d.models[r.model].mesh_count) return 0;
	const uint64_t at = (uint64_t)r.material_offset + mesh_idx;
	return at < d.n_mesh_materials ? d.material_index[at] : 0u;
}
__device__ __forceinline__ float lod_of(const DrawDevice& d, uint32_t e) { return e < d.n_entities ? d.inst[e].lod : 0.0f; }

__device__ __forceinline__ uint32_t kind_of_head(const DrawDevice& d, uint32_t h) {
	const uint32_t type = type_of(d.values[h]);
	if (type == LMX_DRAW_MESH && !(d.flags[h] & DRAW_F_U)) return LMX_RUN_MOVED_MESH;
	return type;
}
__device__ __forceinline__ uint32_t stride_of(uint32_t kind) {
	return kind == LMX_RUN_MESH ? 48u : kind == LMX_RUN_MOVED_MESH ? 96u : kind == LMX_RUN_SKINNED ? 92u : kind == LMX_RUN_DECAL ? 52u : kind == LMX_RUN_CURVE_DECAL ? 68u : 0u;
}

__device__ __forceinline__ void decal_half_extents(const DrawDevice& d, uint32_t kind, uint32_t e, float he[3]) {
	he[0] = he[1] = he[2] = 0.0f;
	if (kind == LMX_RUN_DECAL) {
		if (d.decals && e < d.n_decals) for (int k = 0; k < 3; ++k) he[k] = d.decals[e].half_extents[k];
	} else if (d.curves && e < d.n_curves) {
		for (int k = 0; k < 3; ++k) he[k] = d.curves[e].half_extents[k];
	}
}

// Pass 4 (behind run_of = exclusive sum of head): the first pair of every run.
__global__ __launch_bounds__(DRAW_TILE) void k_draw_run_starts(DrawDevice d) {
	const uint32_t i = blockIdx.x * DRAW_TILE + threadIdx.x;
	if (i < d.n && d.head[i]) d.run_start[d.run_of[i]] = i;
	if (i == d.n) d.run_start[d.run_of[d.n]] = d.n;
}

// Pass 5: per pair of a decal run the near-plane bit (front = does not intersect), per run the aligned size of its slice.
__global__ __launch_bounds__(DRAW_TILE) void k_draw_runs(DrawDevice d, DrawViewDevice v) {
	const uint32_t i = blockIdx.x * DRAW_TILE + threadIdx.x;
	if (i > d.n) return;
	if (i == d.n) {
		d.front[i] = 0;
		return;
	}
	const uint32_t r = d.run_of[i + 1] - 1u; // heads up to and including i
	const uint32_t h = d.run_start[r];
	const uint32_t kind = kind_of_head(d, h);
	uint32_t front = 0;
	if (kind == LMX_RUN_DECAL || kind == LMX_RUN_CURVE_DECAL) {
		const uint32_t e = (uint32_t)d.values[i] & 0x00ffffffu; // :3214, :3276
		const DrawTr t = load_tr(d, e);
		float he[3];
		decal_half_extents(d, kind, e, he);
		const float mb = he[1] > he[2] ? he[1] : he[2]; // maximum(x, y, z), core/math.h:472-475
		const float m = he[0] > mb ? he[0] : mb;
		const float radius = m * 1.73205080757f; // SQRT3
		const float x = (float)(t.px - v.origin[0]), y = (float)(t.py - v.origin[1]), z = (float)(t.pz - v.origin[2]);
		float distance = ((v.nx * x + v.ny * y) + z * v.nz) + v.nd;
		distance = distance < 0 ? -distance : distance;
		front = distance < radius ? 0u : 1u;
	}
	d.front[i] = front;
	if (i == h) {
		const uint32_t count = d.run_start[r + 1] - h;
		d.run_bytes[r] = (count * stride_of(kind) + 15u) & ~15u;
	}
}

__device__ __forceinline__ void store_words(uint8_t* dst, const uint32_t* w, uint32_t n_words) {
	if (n_words % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
		uint4* o = reinterpret_cast<uint4*>(dst);
#pragma unroll
		for (uint32_t k = 0; k < 6; ++k)
			if (4 * k < n_words) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
	} else {
		uint32_t* o = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
		for (uint32_t k = 0; k < 24; ++k)
			if (k < n_words) o[k] = w[k];
	}
}

// Pass 6 (behind the sums of front and run_bytes): one pair per lane - its record; a run's head also writes the run record, its last pair
// the slice's padding (zeros).
__global__ __launch_bounds__(DRAW_TILE) void k_draw_encode(DrawDevice d, DrawViewDevice v) {
	const uint32_t i = blockIdx.x * DRAW_TILE + threadIdx.x;
	if (i == 0) {
		d.counts[0] = d.run_of[d.n];
		d.counts[1] = d.run_offset[d.n];
		d.counts[2] = d.n;
		d.counts[3] = d.n_group_values;
	}
	if (i >= d.n) return;
	const uint32_t r = d.run_of[i + 1] - 1u;
	const uint32_t h = d.run_start[r], end = d.run_start[r + 1];
	const uint32_t count = end - h;
	const uint32_t kind = kind_of_head(d, h);
	const uint32_t stride = stride_of(kind);
	const uint64_t hv = d.values[h];
	const uint32_t head_entity = (uint32_t)hv, mesh_idx = (uint32_t)(hv >> LMX_SORT_VALUE_MESH_IDX_SHIFT);
	const uint32_t offset = d.run_offset[r];
	const uint32_t front_count = d.front_sum[end] - d.front_sum[h];
	if (i == h) {
		LmxDrawRun run;
		run.kind = kind;
		run.bucket = (uint32_t)(d.keys[h] >> LMX_SORT_KEY_BUCKET_SHIFT);
		run.batch = h / d.step;
		run.first_pair = h;
		run.pair_count = count;
		run.data_offset = offset;
		run.stride = stride;
		run.head_entity = head_entity;
		run.mesh_idx = mesh_idx;
		run.front_count = (kind == LMX_RUN_DECAL || kind == LMX_RUN_CURVE_DECAL) ? front_count : count;
		run.group = 0;
		run.total_count = count;
		if (kind == LMX_RUN_AUTOINSTANCED) { // :3006-3012 (one instancer: the group index is the mesh sort key, 24 bits)
			const uint32_t g = head_entity & 0x00ffffffu;
			uint32_t from = 0, to = 0;
			if (d.group_offset && g < d.n_groups) {
				from = d.group_offset[g];
				to = d.group_offset[g + 1];
			}
			run.group = g;
			run.total_count = to - from;
			run.data_offset = 48u * from;
			run.stride = 48;
			run.head_entity = 0;
			run.mesh_idx = 0;
			if (to > from) {
				const uint64_t first = d.group_values[from];
				run.head_entity = (uint32_t)first;
				run.mesh_idx = (uint32_t)(first >> LMX_SORT_VALUE_MESH_IDX_SHIFT);
			}
		}
		d.runs[r] = run;
	}
	if (!stride) return;
	uint32_t w[24];
	uint32_t at = i - h; // record index inside the slice
	const uint32_t raw = (uint32_t)d.values[i];
	if (kind == LMX_RUN_MESH || kind == LMX_RUN_MOVED_MESH) {
		const uint32_t e = raw;
		const DrawTr t = load_tr(d, e);
		const uint32_t lod_d = __float_as_uint(lod_of(d, e) - mesh_lod_of(d, head_entity, mesh_idx));
		w[0] = t.rot[0]; w[1] = t.rot[1]; w[2] = t.rot[2]; w[3] = t.rot[3];
		w[4] = rel_bits(t.px, v.cam[0]); w[5] = rel_bits(t.py, v.cam[1]); w[6] = rel_bits(t.pz, v.cam[2]);
		w[7] = lod_d;
		w[8] = t.scale[0]; w[9] = t.scale[1]; w[10] = t.scale[2];
		if (kind == LMX_RUN_MESH) {
			w[11] = material_of(d, head_entity, mesh_idx); // material->getIndex() of the HEAD's mesh material, :3114
		} else {
			const DrawTr p = load_uploaded(d.prev, d.n_prev, e); // ModelInstance::prev_frame_transform
			w[11] = 0; // padding, :3071
			w[12] = p.rot[0]; w[13] = p.rot[1]; w[14] = p.rot[2]; w[15] = p.rot[3];
			w[16] = rel_bits(p.px, v.cam[0]); w[17] = rel_bits(p.py, v.cam[1]); w[18] = rel_bits(p.pz, v.cam[2]);
			w[19] = lod_d;
			w[20] = p.scale[0]; w[21] = p.scale[1]; w[22] = p.scale[2];
			w[23] = material_of(d, e, mesh_idx); // mi2->mesh_materials[mesh_idx].material_index, :3077
		}
	} else if (kind == LMX_RUN_SKINNED) {
		const uint32_t e = raw;
		const DrawTr t = load_tr(d, e);
		const DrawTr p = load_uploaded(d.prev, d.n_prev, e);
		w[0] = material_of(d, e, mesh_idx);
		w[1] = d.bones_handle && e < d.n_bones ? d.bones_handle[e] : 0u;
		w[2] = d.bones_offset && e < d.n_bones ? d.bones_offset[e] : 0u;
		w[3] = rel_bits(t.px, v.cam[0]); w[4] = rel_bits(t.py, v.cam[1]); w[5] = rel_bits(t.pz, v.cam[2]);
		w[6] = t.rot[0]; w[7] = t.rot[1]; w[8] = t.rot[2]; w[9] = t.rot[3];
		w[10] = t.scale[0]; w[11] = t.scale[1]; w[12] = t.scale[2];
		w[13] = rel_bits(p.px, v.cam[0]); w[14] = rel_bits(p.py, v.cam[1]); w[15] = rel_bits(p.pz, v.cam[2]);
		w[16] = p.rot[0]; w[17] = p.rot[1]; w[18] = p.rot[2]; w[19] = p.rot[3];
		w[20] = p.scale[0]; w[21] = p.scale[1]; w[22] = p.scale[2];
	} else { // DECAL / CURVE_DECAL: front part upwards, back part downwards from the slice's end, in walk order (:3221-3227)
		const uint32_t e = raw & 0x00ffffffu;
		const DrawTr t = load_tr(d, e);
		const uint32_t front_rank = d.front_sum[i] - d.front_sum[h];
		at = d.front[i] ? front_rank : count - 1u - ((i - h) - front_rank);
		w[0] = rel_bits(t.px, v.cam[0]); w[1] = rel_bits(t.py, v.cam[1]); w[2] = rel_bits(t.pz, v.cam[2]);
		w[3] = t.rot[0]; w[4] = t.rot[1]; w[5] = t.rot[2]; w[6] = t.rot[3];
		for (int k = 7; k < 17; ++k) w[k] = 0;
		if (kind == LMX_RUN_DECAL) {
			if (d.decals && e < d.n_decals) {
				const uint32_t* s = reinterpret_cast<const uint32_t*>(d.decals + e);
				for (int k = 0; k < 5; ++k) w[7 + k] = s[k];
			}
			w[12] = d.decals && head_entity < d.n_decals ? d.decals[head_entity].material_index : 0u; // the HEAD's material, :3194 / :3226
		} else {
			if (d.curves && e < d.n_curves) {
				const uint32_t* s = reinterpret_cast<const uint32_t*>(d.curves + e);
				for (int k = 0; k < 9; ++k) w[7 + k] = s[k];
			}
			w[16] = d.curves && head_entity < d.n_curves ? d.curves[head_entity].material_index : 0u;
		}
	}
	uint8_t* slice = d.instance_data + offset;
	store_words(slice + (size_t)at * stride, w, stride / 4);
	if (i + 1 == end) { // the slice's tail up to its 16-byte boundary
		uint32_t* pad = reinterpret_cast<uint32_t*>(slice + (size_t)count * stride);
		const uint32_t n_pad = (((count * stride + 15u) & ~15u) - count * stride) / 4;
		for (uint32_t k = 0; k < n_pad; ++k) pad[k] = 0;
	}
}

// The "fill instance data" block (:3970-4014): one lane per renderable of the instancer CSR; its group from the offsets (binary search),
// Mesh::lod from the group's FIRST renderable (:3983-3990), the material index from the entity's own mesh material (:4007).
__global__ __launch_bounds__(DRAW_TILE) void k_draw_groups(DrawDevice d, DrawViewDevice v) {
	const uint32_t j = blockIdx.x * DRAW_TILE + threadIdx.x;
	if (j >= d.n_group_values) return;
	uint32_t lo = 0, hi = d.n_groups; // the last k with group_offset[k] <= j
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (d.group_offset[mid] <= j) lo = mid;
		else hi = mid;
	}
	const uint64_t first = d.group_values[d.group_offset[lo]];
	const uint32_t first_entity = (uint32_t)first & 0x00ffffffu, mesh_idx = (uint32_t)(first >> LMX_SORT_VALUE_MESH_IDX_SHIFT);
	const uint32_t e = (uint32_t)d.group_values[j];
	const DrawTr t = load_tr(d, e);
	uint32_t w[12];
	w[0] = t.rot[0]; w[1] = t.rot[1]; w[2] = t.rot[2]; w[3] = t.rot[3];
	w[4] = rel_bits(t.px, v.cam[0]); w[5] = rel_bits(t.py, v.cam[1]); w[6] = rel_bits(t.pz, v.cam[2]);
	w[7] = __float_as_uint(lod_of(d, e) - mesh_lod_of(d, first_entity, mesh_idx));
	w[8] = t.scale[0]; w[9] = t.scale[1]; w[10] = t.scale[2];
	w[11] = material_of(d, e, mesh_idx);
	uint4* o = reinterpret_cast<uint4*>(d.group_data + (size_t)j * 48);
	o[0] = make_uint4(w[0], w[1], w[2], w[3]);
	o[1] = make_uint4(w[4], w[5], w[6], w[7]);
	o[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

uint32_t tiles_of(uint32_t n) { return (n + DRAW_TILE - 1) / DRAW_TILE; }

} // namespace

hipError_t launch_draw_flags(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v) {
	const uint32_t n_tiles = tiles_of(d.n);
	hipLaunchKernelGGL(k_draw_flags, dim3(n_tiles), dim3(DRAW_TILE), 0, s, d, v);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_draw_tile_scan, dim3(1), dim3(DRAW_TILE), 0, s, d, n_tiles);
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_draw_heads, dim3(tiles_of(d.n + 1)), dim3(DRAW_TILE), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_draw_runs(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v) {
	hipLaunchKernelGGL(k_draw_run_starts, dim3(tiles_of(d.n + 1)), dim3(DRAW_TILE), 0, s, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_draw_runs, dim3(tiles_of(d.n + 1)), dim3(DRAW_TILE), 0, s, d, v);
	return hipGetLastError();
}

hipError_t launch_draw_encode(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v) {
	hipLaunchKernelGGL(k_draw_encode, dim3(tiles_of(d.n)), dim3(DRAW_TILE), 0, s, d, v);
	return hipGetLastError();
}

hipError_t launch_draw_groups(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v) {
	if (!d.n_group_values) return hipSuccess;
	hipLaunchKernelGGL(k_draw_groups, dim3(tiles_of(d.n_group_values)), dim3(DRAW_TILE), 0, s, d, v);
	return hipGetLastError();
}

} // namespace lmx
