// lmx_kernels.h — host-callable launchers of the gfx950 kernels (defined in *_kernels.hip) + shared device layouts.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmx_math.h"
#include "lmx_types.h"
#include "lmx_controller_program.h"

// Dynamic LDS of a launch. (tests/hostsim compiles these sources for the CPU and supplies its own definition: there the block is
// a buffer of the simulated device, not an `extern __shared__` array.)
#ifndef LMX_DYNAMIC_LDS
#define LMX_DYNAMIC_LDS(T, name) extern __shared__ T name[]
#endif

namespace lmx {

constexpr int MAX_FRUSTA = 8;
constexpr int MAX_TYPES = 8;
constexpr uint32_t CHUNK = 64;          // spheres per chunk = one wavefront
constexpr uint32_t TILE_ALIGN = 4096;   // type ranges are padded to this many spheres (largest tile of any variant)
constexpr uint32_t CELL_DEAD = 0x80000000u;

// One (cell index, type, is_big) group. meta = type | is_big << 8 | CELL_DEAD.
struct CellKey { int32_t ix, iy, iz; uint32_t meta; };
// The same group in 8 bytes, relative to its TILE's box (TileBox::lo): xy = dx | dy << 16, zf = dz | flags << 16 with flags bit 0 = is_big,
// bit 15 = dead. The per-tile cell tables are the largest part of what k_cull_tile reads besides the spheres and ids themselves (16 B x ~1 M
// cells per 10 M entities, padded per tile: 18.7 of the launch's 224.5 MB); the type is not needed on the device (the tile's shard says it).
struct PackedCellKey { uint32_t xy, zf; };
constexpr uint32_t PACKED_CELL_BIG = 1u << 16, PACKED_CELL_DEAD = 1u << 31;
// Header of a 64-sphere chunk: cell slot of its first sphere, bit l of flags = "sphere l starts the next cell".
struct ChunkHdr { uint32_t cell, pad; uint64_t flags; };

// Per-type ranges in the padded slot space of one set (static or dynamic) + the type's output shards.
struct TypeTable {
	uint32_t ent_start[MAX_TYPES];   // first slot of the type (static set: multiple of TILE_ALIGN, dynamic set: of 2048)
	uint32_t ent_end[MAX_TYPES];     // end of the padded range
	uint32_t shard_first[MAX_TYPES]; // global index of the first output shard the type's tiles of this set reserve from
	uint32_t shard_n[MAX_TYPES];     // number of shards: block b (TILE_ALIGN slots) of the type uses shard_first + b % shard_n
};

struct FrustaArg { DevFrustum f[MAX_FRUSTA]; };

struct CullDeviceView {
	const float4* spheres;       // [n_padded] {rel.x, rel.y, rel.z, radius}, cell-relative fp32 (culling_system.cpp:100)
	const int32_t* ids;          // [n_padded] entity index, -1 for padding and removed entities
	const ChunkHdr* hdr;         // [n_padded / 64]
	uint32_t n_padded;
	// per tile-size variant k (tile = 4096 >> k): tile-major cell keys + {first cell, n cells} + cell-index box per tile
	const CellKey* tile_cells[3];   // 16-byte keys - or, keys_packed, 8-byte ones (PackedCellKey) behind the same pointers
	bool keys_packed;               // every tile's cells lie within 65535 cell indices of its box's low corner on every axis (any real scene)
	const uint32_t* tile_tab[3];
	const TileBox* tile_box[3];
	uint32_t tile_cap[3];
	// per tile: {output shard, start of that shard's window in an ids row} - what a surviving tile needs to reserve and write (a function of the
	// tile's type range and of the output layout: looked up, it was ~90 scalar instructions incl. an integer modulo, and two dependent loads)
	const uint2* tile_out[3];
};

// Where a cull writes. The visible ids of (frustum f, shard s) go to ids[f * stride + win_base[s] + k], k < the shard's counter
// counts[f * cnt_frustum_stride + s * cnt_pad]; counters sit cnt_pad words apart (own cache line: same-line atomics serialise).
// Every launch also clears counts_next[0 .. n_zero) (the counters of the following cull on this view, ping-pong).
struct CullOut {
	int32_t* ids;
	uint32_t stride;
	const uint32_t* win_base;
	uint32_t* counts;
	uint32_t cnt_pad, cnt_frustum_stride;
	uint32_t* counts_next;
	uint32_t n_zero;
	// profiling only (lmx_profile_enable): the dispatch's OWN begin / end timestamps go into these events (hipExtLaunchKernelGGL) -
	// events recorded around the launch also time ~3 us of command processing per pair, 7 % of a 40 us kernel
	hipEvent_t ev_start = nullptr, ev_stop = nullptr;
	// optional, parallel to `ids` (same stride, same windows): the STATIC-SET SLOT every visible id came from, -1 for ids of the dynamic
	// set. Consumers that keep per-entity tables in slot order (the sort-key kernels) read them with the locality of the sorted set.
	int32_t* slots = nullptr;
};

// k_cull_tile over the static set's slots [ent_begin, ent_end) (multiples of TILE_ALIGN). `variant` picks the form of the 1-frustum kernel
// (both: 4 waves x 8 chunks, 2048-sphere tiles): 1 = streaming (4 chunks' loads in flight per wave), 4 = all 8 in flight; ignored for n_frusta > 1.
size_t cull_tile_lds_bytes(int n_frusta, uint32_t cell_cap);
uint32_t cull_tile_size(int n_frusta, int variant);
hipError_t launch_cull_tile(hipStream_t s, const CullDeviceView& v, uint32_t ent_begin, uint32_t ent_end, const TypeTable& tt,
	const FrustaArg& fr, int n_frusta, const CullOut& out, int variant);

// Dynamic set: entities whose transform changes every frame (bound to the world hierarchy) and entities added / re-celled since
// the last compaction of the static set are kept UNSORTED as world position (fp64) + radius + id. Their cell, cell-relative
// position and per-cell class are recomputed per entity per cull with exactly the arithmetic CullingSystem::set + cullInternal
// would apply (cell_of, classify_cell, sphere_visible), so no re-binning is ever needed.
struct DynDeviceView {
	double* px; double* py; double* pz;
	float* radius;
	int32_t* ids; // -1 = free slot
	uint32_t n_padded;
};
hipError_t launch_dyn_carry_over(hipStream_t s, const DynDeviceView& from, const DynDeviceView& to, const int32_t* new_slot_of_entity, uint32_t n_entities);
hipError_t launch_cull_dynamic(hipStream_t s, const DynDeviceView& d, uint32_t slot_begin, uint32_t slot_end, const TypeTable& dyn_tt,
	const FrustaArg& fr, int n_frusta, const CullOut& out);
uint32_t cull_dynamic_tile(int n_frusta, uint32_t n_slots);

// Patch records staged by the host between two culls (CullingSystem::add / remove / set* are O(1): culling_system.cpp:131-258)
struct PatchSphere { uint32_t slot; float x, y, z, radius; };                 // static set: in-cell move / radius change
struct PatchId { uint32_t slot; int32_t id; };                                 // static set: removal (tombstone, id = -1)
struct PatchDyn { uint32_t slot; int32_t id; float radius; uint32_t pad; double px, py, pz; }; // dynamic set: add / remove / set
// (a tombstone also clears TILE_DENSE of the tiles that hold its slot, in all three tile-size variants)
hipError_t launch_apply_patches(hipStream_t s, float4* spheres, int32_t* ids, TileBox* const tile_box[3], const DynDeviceView& d, const PatchSphere* ps,
	uint32_t n_ps, const PatchId* pi, uint32_t n_pi, const PatchDyn* pd, uint32_t n_pd);

// Per-(frustum, type) totals and per-(frustum, shard) offsets of the consolidated lists: totals[f * MAX_TYPES + t], pref[f * n_shards + s]
// (offset of shard s inside its type's consolidated list). shard_type[s] = renderable type of shard s. packed_start (optional):
// [f * MAX_TYPES + t] = start of type t when the types of a frustum are packed back to back.
hipError_t launch_cull_finalize(hipStream_t s, const uint32_t* counts, uint32_t cnt_pad, uint32_t cnt_frustum_stride, const uint8_t* shard_type,
	uint32_t n_shards, uint32_t n_frusta, uint32_t* totals, uint32_t* pref, uint32_t* packed_start);
// One contiguous list per (frustum, type): dst[f * dst_stride + type_start[f * type_start_stride + type] + pref + k] = src[f * src_stride + win_base[s] + k],
// clipped to dst_cap ids per frustum row
// finalize + consolidate in one launch, into the packed record [MAX_TYPES counts | ids, types back to back] of each of n_frusta frusta
// (frustum f: ids row src + f * src_stride, counters counts + f * cnt_stride, record header / dst + f * rec_stride; strides in words)
hipError_t launch_cull_pack(hipStream_t s, const int32_t* src, const uint32_t* win_base, const uint32_t* counts, uint32_t cnt_pad, const uint8_t* shard_type,
	uint32_t n_shards, uint32_t max_shard_cap, uint32_t* header, int32_t* dst /* behind the header */, uint32_t dst_cap, uint32_t n_frusta = 1,
	uint32_t src_stride = 0, uint32_t cnt_stride = 0, uint32_t rec_stride = 0);
// the same with a place and a capacity PER record: record f = [MAX_TYPES counts | lay.cap[f] ids] at rec_base + lay.off[f] (words)
struct PackLayout {
	uint64_t off[MAX_FRUSTA];
	uint32_t cap[MAX_FRUSTA];
};
hipError_t launch_cull_pack_layout(hipStream_t s, const int32_t* src, const uint32_t* win_base, const uint32_t* counts, uint32_t cnt_pad, const uint8_t* shard_type,
	uint32_t n_shards, uint32_t max_shard_cap, int32_t* rec_base, const PackLayout& lay, uint32_t n_frusta, uint32_t src_stride, uint32_t cnt_stride);
hipError_t launch_cull_consolidate(hipStream_t s, const int32_t* src, uint32_t src_stride, const uint32_t* win_base, const uint32_t* counts,
	uint32_t cnt_pad, uint32_t cnt_frustum_stride, const uint8_t* shard_type, const uint32_t* type_start /* device */, uint32_t type_start_stride,
	const uint32_t* pref, uint32_t n_shards, uint32_t n_frusta, uint32_t max_shard_cap, int32_t* dst, uint32_t dst_stride, uint32_t dst_cap, const int32_t* src2 = nullptr /* a second array with the same windows, gathered by the same launch */, int32_t* dst2 = nullptr);

// ---- world transforms ------------------------------------------------------------------------------------
struct WorldDevice {
	// slot order = (level, parent slot); all arrays [n]
	double* lpx; double* lpy; double* lpz; float4* lrot; float* lsx; float* lsy; float* lsz; // local (roots: unused)
	double* wpx; double* wpy; double* wpz; float4* wrot; float* wsx; float* wsy; float* wsz; // world
	const int32_t* parent_slot; // -1 for roots
	uint8_t* dirty;             // XF_* mark per slot: what was staged since the last propagation
};
enum : uint8_t { XF_CLEAN = 0, XF_SET_LOCAL = 1, XF_SET_WORLD = 2, XF_MOVED = 4 };
enum { XF_STAGE_RAW = 0, XF_STAGE_RAW_WORLD = 1, XF_STAGE_SET_LOCAL = 2, XF_STAGE_SET_WORLD = 3 };
// world[s] = compose(world[parent_slot[s]], local[s]) for s in [first, first + n)
hipError_t launch_xform_level(hipStream_t s, const WorldDevice& w, uint32_t first, uint32_t n);
// out[entity_of_slot[s]] = AoS Transform (56 B) for s in [0, n)
hipError_t launch_xform_export(hipStream_t s, const WorldDevice& w, const int32_t* entity_of_slot, uint32_t n, void* out_transforms);
// every level in ONE launch (k_xform_subtree): run r of consecutive roots owns slots [table[r * n_levels + l], table[(r + 1) * n_levels + l]) of
// level l. The block also clears its marks, appends its moved nodes to the hand-back lists (count != nullptr) and refreshes the culling
// spheres of its bound entities (bound_dyn_of_slot != nullptr: dynamic-set index per slot or 0xffffffff, model radius per slot).
constexpr uint32_t XF_SUBTREE_NODES = 1024;      // nodes a run aims at (4 per thread of its block)
constexpr uint32_t XF_SUBTREE_MAX_RUN = 16384;   // ... and the most one root's subtree may hold before the per-level launches take over
constexpr uint32_t XF_SUBTREE_MAX_LEVELS = 16;
struct XformSubtree {
	const uint32_t* table;
	uint32_t n_levels;
	const int32_t* entity_of_slot;
	uint32_t cap;
	int32_t* out_entity;
	void* out_tr; // Transform AoS, 56 B
	uint32_t* count;
	const uint32_t* bound_dyn_of_slot;
	const float* bound_radius_of_slot;
	double *dyn_px, *dyn_py, *dyn_pz;
	float* dyn_radius;
};
hipError_t launch_xform_subtree(hipStream_t s, const WorldDevice& w, const XformSubtree& a, uint32_t n_runs);
// append {entity, world transform} of every slot marked XF_MOVED to the lists (ballot-compacted, one atomic per wave) and clear all marks
hipError_t launch_xform_collect_moved(hipStream_t s, const WorldDevice& w, const int32_t* entity_of_slot, uint32_t n, uint32_t cap, int32_t* out_entity,
	void* out_transforms, uint32_t* count);
// stage transforms (AoS LmxTransform, device memory) into the SoA arrays; mode = XF_STAGE_* (see k_xform_scatter)
hipError_t launch_xform_scatter(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const int32_t* entity,
	const void* transforms, uint32_t n, int mode);
// culling refresh for bound entities (RenderModuleImpl::onModelInstanceMoved, render_module.cpp:1544-1554): the dynamic
// set's position / radius of bound entity i become (world.pos, model_radius[i] * maximum(scale.x, scale.y, scale.z))
hipError_t launch_sphere_refresh(hipStream_t s, const WorldDevice& w, const uint32_t* bound_slot, const uint32_t* bound_dyn,
	const float* model_radius, double* dyn_px, double* dyn_py, double* dyn_pz, float* dyn_radius, uint32_t n);

// ---- skinning --------------------------------------------------------------------------------------------
struct SkinInstance {
	uint32_t bone_offset;  // into pose arrays / palette (in bones)
	uint32_t n_bones;
	uint32_t model_offset; // into parents / inverse bind arrays (in bones)
	int32_t first_nonroot;
	uint32_t vert_offset;  // into mesh vertex arrays
	uint32_t n_verts;
	uint32_t out_offset;   // into output vertex array (in vertices)
	uint32_t max_depth;    // deepest bone level of the model (root = 0)
	uint32_t lv_items_offset; // into level_items: the model's bones >= first_nonroot sorted by depth, as bone | parent << 16
	uint32_t lv_off_offset;   // into level_off: max_depth + 1 offsets (bones of depth d = [off[d-1], off[d]))
};
// k_skin_shared work item: instances [first_inst, first_inst + count) share mesh and bone count; vertices [v_begin, v_end) of it
// (the tile's records live in the mesh table with TILE-LOCAL bone indices: rec_offset = the mesh's first record there, in vertices;
// tile_bones[bones_at .. + n_tile_bones) = the model bones the tile references, in local-index order)
struct SkinChunk { uint32_t first_inst, count, v_begin, v_end, rec_offset, bones_at, n_tile_bones, pad; };
struct PoseGroup { uint32_t first_inst; uint32_t count; }; // consecutive instances of one model, count <= 4 / 2 / 1 by bone count (<= 64 / 128 / 196)
#ifndef LMX_POSE_GROUP_SHIFT
#define LMX_POSE_GROUP_SHIFT 2
#endif
constexpr int POSE_GROUP_SHIFT = LMX_POSE_GROUP_SHIFT; // log2 of the instances per group of the smallest bone-count class; halves per class (k_pose_palette, skin_kernels.hip)
constexpr uint32_t POSE_GROUP_CAP = 1u << POSE_GROUP_SHIFT;
// ---- bone attachments (xform_kernels.hip) ----
struct BoneAttachDevice { uint32_t slot, parent_slot, skin_instance, bone; float rel_pos[3]; float rel_rot[4]; };
hipError_t launch_bone_attach(hipStream_t s, const WorldDevice& w, const BoneAttachDevice* att, uint32_t n, const SkinInstance* inst,
	const float* pose_pos, const float4* pose_rot);

// ---- world edits (world_edit_kernels.hip): destroy / create / re-parent a batch, then the slot order again from `parent` ----
struct WorldEditDevice {
	int32_t* parent; // by entity, -1: root (dead entities are childless roots)
	uint8_t* alive;  // by entity
	uint8_t* mark;   // by entity, zero on entry: the destroy list's entities
	uint8_t* kill;   // by entity, zero on entry: dies in this call
};
struct WorldEditOrder {
	const uint32_t* sorted; // entities sorted by (parent + 1, entity): the roots, then every parent's children
	const uint32_t* first;  // [n + 1] by parent + 1: where that group begins in `sorted`
	const uint32_t* count;  // [n + 1] its size
	int32_t* entity_of_slot;
	int32_t* slot_of_entity;
	int32_t* parent_slot;
	uint32_t* root_of_slot;
};
constexpr uint32_t WORLD_EDIT_SMALL_LEVEL = 256; // a level of at most this many slots expands in one block (lmx_wave.h's block_scan)
hipError_t launch_edit_kill(hipStream_t s, const WorldEditDevice& d, const int32_t* destroy, uint32_t n_destroy, uint32_t n_old);
hipError_t launch_edit_link(hipStream_t s, const WorldEditDevice& d, const int32_t* create, uint32_t n_create, const int32_t* child, const int32_t* new_parent, uint32_t n_reparent);
hipError_t launch_edit_keys(hipStream_t s, const WorldEditDevice& d, uint32_t n, uint32_t* key, uint32_t* value, uint32_t* n_live /* += live entities */);
hipError_t launch_edit_child_ranges(hipStream_t s, const uint32_t* sorted_key, uint32_t n, uint32_t* first /* [n + 1] */, uint32_t* count /* [n + 1], zero on entry */);
hipError_t launch_edit_roots(hipStream_t s, const WorldEditOrder& o, uint32_t n_roots);
// level [level_first, level_first + m) -> its children behind it; the small form writes the next level's size to *total
hipError_t launch_edit_level_small(hipStream_t s, const WorldEditOrder& o, uint32_t level_first, uint32_t m, uint32_t* total);
hipError_t launch_edit_level_count(hipStream_t s, const WorldEditOrder& o, uint32_t level_first, uint32_t m, uint32_t* cnt /* [m + 1], the last one 0 */);
hipError_t launch_edit_level_scatter(hipStream_t s, const WorldEditOrder& o, uint32_t level_first, uint32_t m, const uint32_t* cnt, const uint32_t* off);
hipError_t launch_edit_permute(hipStream_t s, const WorldDevice& from, const WorldDevice& to, const int32_t* entity_of_slot, const int32_t* old_slot_of_entity, const uint8_t* kill /* by entity: died in this call */,
	uint32_t n_old, uint32_t n, const uint32_t* dyn_from, const float* radius_from, uint32_t* dyn_to /* nullptr: no per-slot culling tables */, float* radius_to);
hipError_t launch_edit_create(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const int32_t* create, const void* transforms, uint32_t n);
hipError_t launch_edit_locals(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const int32_t* child, const int32_t* new_parent, uint32_t n);
hipError_t launch_edit_remap(hipStream_t s, const int32_t* old_entity_of_slot, const int32_t* slot_of_entity, const uint8_t* kill, uint32_t* bound_slot, uint32_t n_bound,
	BoneAttachDevice* attach, uint32_t n_attach);
// dropped[0 .. *count) = the entries of the binding list whose entity dies in this call (any order); *count zero on entry
hipError_t launch_edit_dropped(hipStream_t s, const int32_t* old_entity_of_slot, const uint8_t* kill, const uint32_t* bound_slot, uint32_t n_bound, uint32_t* dropped,
	uint32_t* count);
hipError_t launch_edit_root_sizes(hipStream_t s, const uint32_t* root_of_slot, const uint32_t* level_start, uint32_t n_levels, uint32_t n_roots, uint32_t* size);
hipError_t launch_edit_run_table(hipStream_t s, const uint32_t* root_of_slot, const uint32_t* level_start, uint32_t n_levels, const uint32_t* run_root, uint32_t n_rows,
	uint32_t* table);

// ---- animation sampling (anim_kernels.hip) ----
struct AnimDevice { // one Animation resource: offsets into the concatenated tables of AnimTables
	float fps;
	uint32_t frame_count, length, tfs_bits, rfs_bits;
	uint32_t max_bone;                 // m_max_accessed_bone_index
	uint32_t src_off;                  // 2 * (max_bone + 1) int32: translation / rotation source per bone
	uint32_t ct_off, tt_off, cr_off, rt_off;
	uint32_t tstream_off, rstream_off; // bytes, 8-byte aligned
	int32_t root_translation_track, root_rotation_track;
	uint32_t root_off;                 // frames, into root_translations / root_rotations
};
struct AnimTables {
	const int32_t* src;
	const LmxAnimConstTranslation* const_translations;
	const LmxAnimTranslationTrack* translations;
	const LmxAnimConstRotation* const_rotations;
	const LmxAnimRotationTrack* rotations;
	const uint8_t *translation_stream, *rotation_stream;
	const float* root_translations;
	const float4* root_rotations;
};
hipError_t launch_anim_update(hipStream_t s, const SkinInstance* inst, uint32_t n_inst, const AnimDevice* anims, const AnimTables& t,
	const uint32_t* anim_of_instance, uint32_t* time_of_instance, float time_delta, float weight, const float* model_rel_pos,
	const float4* model_rel_rot, float* pose_pos, float4* pose_rot);
hipError_t launch_anim_blend_stack(hipStream_t s, const SkinInstance* inst, uint32_t n_inst, const AnimDevice* anims, const AnimTables& t, uint32_t n_anims,
	const LmxBlendSample* samples, const uint32_t* first_sample, const float* model_rel_pos, const float4* model_rel_rot, float* pose_pos, float4* pose_rot);
// evalBlendStack with IK: `parents` = the bone parents of every skin model, by model bone offset (SkinInstance::model_offset)
hipError_t launch_anim_blend_instrs(hipStream_t s, const SkinInstance* inst, uint32_t n_inst, const AnimDevice* anims, const AnimTables& t, uint32_t n_anims,
	const LmxBlendInstr* instrs, const uint32_t* first_instr, const int16_t* parents, const float* model_rel_pos, const float4* model_rel_rot, float* pose_pos,
	float4* pose_rot);

// ---- animator controllers (animator_kernels.hip): Controller::update of every Animator, the VM of lmx_controller_program.h ----
struct CtlHeader { uint32_t nodes_off, ops_off, exprs_off, aux_off, root, n_inputs, state_words, max_instrs; }; // one controller in the concatenated program tables
struct CtlAnimator {       // one Animator = one skin instance that has a controller
	uint32_t controller;   // LMX_CONTROLLER_NONE: the lane order does not list it
	uint32_t slots_off;    // RuntimeContext::animations of its (controller, set)
	uint32_t state_base;   // its column of the runtime-data words: word k at state[state_base + k * state_stride]
	uint32_t state_stride; // the Animators of its controller (they are neighbours in the lane order, so a wave reads a word of 64 of them at once)
	uint32_t input_base;   // in 16-byte Value records
	uint32_t instr_base;   // its max_instrs records of the instruction slots
	uint32_t ik_off;       // the resolved leaf bones of its (controller, model)
	uint32_t flags;
};
struct AnimatorTables {
	const CtlHeader* headers;
	const CtlNode* nodes;
	const CtlOp* ops;
	const uint32_t *exprs, *aux, *slots, *ik_leaf;
	const CtlClip* clips;
	const float *rm_t, *rm_r;
};
// lane p runs Animator order[p]: state_in -> state_out (+ state_len words), root_motion (7 floats each, read for the stale value and written),
// slots_out[instr_base ..] and counts
hipError_t launch_animators_update(hipStream_t s, const AnimatorTables& t, const CtlAnimator* animators, const uint32_t* order, uint32_t n_active, const uint32_t* inputs,
	const uint32_t* state_in, uint32_t* state_out, uint32_t* state_len, float* root_motion, LmxBlendInstr* slots_out, uint32_t* counts, uint32_t time_delta);
// the slots' records into the first_instr form of k_anim_blend_instrs (first = exclusive scan of counts); `samples` (optional): their SAMPLE
// fields in the 16-byte form of k_anim_blend_stack as well, for a call in which no record can be an IK
hipError_t launch_animators_pack(hipStream_t s, const CtlAnimator* animators, uint32_t n, const uint32_t* first, const uint32_t* counts, const LmxBlendInstr* slots_out,
	LmxBlendInstr* packed, LmxBlendSample* samples);
// RuntimeContext::inputs from device memory: the payloads of `values`, typed as the controllers declare them
hipError_t launch_animators_set_inputs(hipStream_t s, const uint32_t* values, const uint32_t* types, uint32_t* inputs, uint32_t n_records);
// animation_module.cpp:630-635 for the listed Animators: world transforms of `entity` advanced by root_motion into `out` (LmxTransform records)
hipError_t launch_animators_root_motion(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const uint32_t* animator, const int32_t* entity, uint32_t n,
	const float* root_motion, void* out);

// ---- createSortKeys (keys_kernels.hip) ----
// Counter words. {pairs, recs} and {poses, dirty} are two 64-bit cells on their own 128-byte lines: k_keys_mesh reserves a tile's four
// output ranges with two returning atomics on two lines instead of four on one (measured: no change of the kernel's 124 us per
// million visible entities - it is bound by its random 64-byte gathers and line write-backs, see DESIGN.md - but half the atomics).
enum { KEYS_N_PAIRS = 0, KEYS_N_RECS = 1, KEYS_N_POSES = 32, KEYS_N_DIRTY = 33, KEYS_OVERFLOW = 64, KEYS_N_GROUPS = 96, KEYS_COUNTERS = 128 };
struct KeysViewDevice { // what the kernels read of a LmxKeysView, bucket_map as built at pipeline.cpp:3802-3812
	uint32_t bucket_map[255];
	uint8_t layer_to_bucket[255];
	uint8_t is_shadow;
	double cam[3], ref[3];
	float lod_multiplier_rcp, time_delta;
	uint32_t frame_number;
};
// ModelInstance {model, mesh_materials, lod, flags, dirty, pose->frame} + World::getTransforms()[e].pos, one cache-line-friendly record
struct alignas(64) KeysInstance {
	double pos[3];
	int32_t model;            // -1: the entity has no model instance
	uint32_t material_offset;
	float lod;
	uint32_t pose_frame;
	uint8_t flags, dirty;
	uint8_t pad[22];
};
static_assert(sizeof(KeysInstance) == 64, "one record per 64-byte sector");
struct KeysSlotState { float lod; uint32_t pose_frame; };
// (LMX_KEYS_OPT_SPLIT_STATE = 2, the default since round 4: createSortKeys 138 -> 129 us on the round-3 driver box) the slot-ordered mirror as a structure of arrays: the 42 bytes of a record the key kernel reads,
// one dense array per field, so that a wave's load of a field is one contiguous run instead of 64 pieces at a 64-byte stride
#ifndef LMX_KEYS_MAX_COPIES
#define LMX_KEYS_MAX_COPIES 256 // copies of the instancer's per-key counters (power of two, <= 256: 8 bits of rec_key)
#endif
struct KeysSoA { double *px, *py, *pz; int32_t* model; uint32_t* material_offset; uint16_t* flags_dirty; /* flags | dirty << 8 */ };
#ifndef LMX_KEYS_SPLIT_STATE_DEFAULT
#define LMX_KEYS_SPLIT_STATE_DEFAULT 2 // initial value of lmx_keys_set_option(LMX_KEYS_OPT_SPLIT_STATE)
#endif
struct KeysDevice {
	// model instances by entity index: ONE 64-byte record per entity (the visible ids are in cell order, entity indices are not:
	// seven separate per-entity arrays meant seven random 128-byte lines per visible entity and made the kernel traffic-bound)
	uint32_t n_entities;
	KeysInstance* inst;       // lod and pose_frame are updated in place
	const LmxMeshMaterial* mesh_materials;
	// the same records in STATIC-SLOT order (the order the cull emits visible ids in), material_offset pointing into mm_s: entities of
	// the sorted set are read with the locality of the set; ids of the dynamic set (slot -1) take the entity-indexed tables above
	KeysInstance* inst_s;
	const LmxMeshMaterial* mm_s;
	// (LMX_KEYS_SPLIT_STATE, experiment) the two fields of a record the kernel WRITES - ModelInstance::lod and Pose::frame - of the sorted
	// set's entities in a dense array of their own, 8 bytes per slot: a 4-byte update of a 64-byte record dirties a whole sector per visible
	// entity (the traffic model of tests/hostsim and the PMC counters agree on ~230 B of traffic per visible entity against 87 algorithmic)
	KeysSlotState* state_s; // nullptr: lod / pose_frame live in inst_s
	KeysSoA soa;            // soa.model != nullptr: the mirror's records are these arrays (inst_s is not allocated), state_s holds lod / pose_frame
	const LmxKeysModel* models;
	const uint32_t *decal_sort_key, *curve_sort_key;
	const uint8_t *decal_layer, *curve_layer;
	// positions: KeysInstance::pos, or the world hierarchy's SoA through slot_of_entity when bound
	const double *wpx, *wpy, *wpz;
	const int32_t* slot_of_entity;
	// outputs
	uint64_t *keys, *values;
	uint32_t cap_pairs;
	uint32_t* rec_key;
	uint64_t* rec_value;
	uint32_t cap_recs;
	uint32_t max_sort_key;
	// auto-instancer groups. The per-key counters are PRIVATISED: copy c (= block index mod n_copies) has its own count / cursor
	// row, so the atomics of a scene with few distinct mesh sort keys (all of them on a handful of cache lines) spread over
	// n_copies times as many lines. A record remembers its copy in bits 24..31 of rec_key.
	uint32_t n_copies;         // power of two, <= LMX_KEYS_MAX_COPIES
	// Two counter tables take turns (round 5: the chain had a fill of its own): a run's key kernels build the histogram in group_count,
	// which arrives ZERO; k_keys_reduce_copies turns it into per-copy bases (group_base), zeroes it - it is the scatter's cursor table
	// from then on - and zeroes the OTHER table (group_count_next: the previous run's cursors), which is the next run's histogram.
	uint32_t *group_count;      // [n_copies][max_sort_key + 1]: per-copy sizes, then the scatter's cursors
	uint32_t *group_count_next; // the same table of the next run
	uint32_t *group_base;       // [n_copies][max_sort_key + 1]: where copy c's records of group k start inside the group
	uint32_t *group_total;      // [max_sort_key + 1]
	uint32_t *group_offset;     // [max_sort_key + 2]
	uint64_t* group_values;
	// block ranks (key ranges that fit k_keys_mesh's LDS histogram; nullptr: the private copies above): every block of k_keys_mesh owns
	// a row [max_sort_key + 1]: per key the records of the blocks that finished before it; a record carries its rank among its block's
	// records of its key (rec_rank) and its row in bits 12..31 of rec_key
	uint32_t* block_rows;
	// ... (key ranges up to 1024; nullptr beyond: k_keys_reduce_rows scans the columns) one counter per key on a cache line of its own: a
	// block adds its row's counts at its end, what the add returns is the row's entry (the records of the key in the blocks before),
	// the counters end up as the groups' sizes. total_pad_next: the next run's, zeroed by this run's last kernel.
	uint32_t *total_pad, *total_pad_next;
	uint32_t cap_rows, n_rows; // rows allocated; rows of this run (= k_keys_mesh's grid: set by launch_keys)
	uint32_t* rec_rank;
	int32_t *poses, *dirty_list;
	uint32_t cap_list;
	uint32_t* counters;       // KEYS_*: arrive zero
	uint32_t* counters_next;  // the next run's (the previous run's results: valid until this run starts), zeroed by k_keys_reduce_copies
};
// The visible ids of ONE renderable type as the cull kernels leave them (lmx_cull_device_shards): `n` shards, shard s holding
// counts[s * cnt_pad] ids at ids + win_base[s] (and their static-set slots at slots + win_base[s]). The key kernels walk the windows
// themselves: gathering them into one list first (k_cull_finalize + k_cull_consolidate) was 14 of the chain's 94 us. win_base == nullptr:
// one contiguous list (n == 1, counts -> its length) - what a type with more than KEYS_MAX_SHARDS shards falls back to.
constexpr int KEYS_PAD_WORDS = 32; // a padded per-key counter: one 128-byte line
constexpr int KEYS_SCATTER_OFFSETS = 1024; // key ranges up to here: k_keys_scatter forms the group offsets itself and (block ranks) the rows' entries come out of returning adds
constexpr int KEYS_MAX_SHARDS = 128; // the layout builder gives a type <= 64 shards for the sorted set + <= 8 for the dynamic one
struct KeysShardList {
	const int32_t* ids;
	const int32_t* slots; // optional
	const uint32_t* counts;
	const uint32_t* win_base;
	uint32_t cnt_pad, n, cap; // cap: an upper bound of the ids (grid size)
};
hipError_t launch_keys_mirror_count(hipStream_t s, const int32_t* slot_ids, uint32_t n_slots, const KeysInstance* inst, uint32_t n_entities, const LmxKeysModel* models, uint32_t* count);
hipError_t launch_keys_mirror_fill(hipStream_t s, const int32_t* slot_ids, uint32_t n_slots, const KeysInstance* inst, uint32_t n_entities, const LmxKeysModel* models,
	const LmxMeshMaterial* mesh_materials, const uint32_t* offset, KeysInstance* inst_s /* or */, const KeysSoA& soa, LmxMeshMaterial* mm_s, KeysSlotState* state_s /* optional */);
hipError_t launch_keys_mirror_positions(hipStream_t s, const int32_t* slot_ids, uint32_t n_slots, const KeysInstance* inst, uint32_t n_entities, KeysInstance* inst_s, const KeysSoA& soa);
hipError_t launch_keys_mirror_sync(hipStream_t s, const int32_t* slot_ids, uint32_t n_slots, const KeysInstance* inst_s, const int32_t* model_s, const KeysSlotState* state_s,
	KeysInstance* inst, uint32_t n_entities);
hipError_t launch_keys_mirror_carry(hipStream_t s, const PatchId* patches, uint32_t n, const int32_t* slot_ids, uint32_t n_slots, const KeysInstance* inst_s, const int32_t* model_s,
	const KeysSlotState* state_s, KeysInstance* inst, uint32_t n_entities);
uint32_t keys_mesh_grid_cap(); // the largest grid of k_keys_mesh = the rows a block-ranks table needs
hipError_t launch_keys(hipStream_t s, const KeysDevice& d, const KeysViewDevice& view, const KeysShardList& meshes, const KeysShardList& decals, const KeysShardList& curves);

// ---- createCommands (draw_kernels.hip): runs + instance records from the sorted pairs, the instancer groups' records ----
struct DrawDecalRec { float half_extents[3]; float uv_scale[2]; uint32_t material_index; uint32_t pad[2]; };               // 32 B
struct DrawCurveRec { float half_extents[3]; float uv_scale[2]; float bezier[4]; uint32_t material_index; uint32_t pad[2]; }; // 48 B
struct DrawViewDevice {
	double cam[3];
	double origin[3];       // ShiftedFrustum::origin
	float nx, ny, nz, nd;   // the NEAR plane (intersectNearPlane, core/geometry.cpp:38-46)
	uint32_t depth_sorted[8]; // bit b: buckets[b].sort == BucketDesc::DEPTH
};
struct DrawDevice {
	// inputs: the sorted pairs, the instancer CSR
	const uint64_t *keys, *values;
	uint32_t n, step;          // pairs; pairs per batch = ceil(n / n_batches)
	const uint32_t* group_offset; // [n_groups + 1], nullptr: no instancer
	const uint64_t* group_values;
	uint32_t n_groups, n_group_values;
	// tables by entity index (every one may be shorter than the entity ids met: what an entity lacks reads as zero)
	const KeysInstance* inst; uint32_t n_entities;
	const LmxKeysModel* models; uint32_t n_models;
	const float* mesh_lod; uint32_t n_meshes;
	const uint32_t* material_index; uint32_t n_mesh_materials;
	const LmxTransform* tr; uint32_t n_tr;       // uploaded transforms, or (tr == nullptr) the world hierarchy in place:
	const double *wpx, *wpy, *wpz; const float4* wrot; const float *wsx, *wsy, *wsz; const int32_t* slot_of_entity; uint32_t n_world;
	const LmxTransform* prev; uint32_t n_prev;
	const uint32_t *bones_handle, *bones_offset; uint32_t n_bones;
	const DrawDecalRec* decals; uint32_t n_decals;
	const DrawCurveRec* curves; uint32_t n_curves;
	// scratch
	uint8_t* flags;        // [n] DRAW_F_*
	uint8_t *tile_fn, *tile_in; // [tiles]
	uint32_t *head, *run_of;   // [n + 1] head flag, its exclusive sum (run_of[n] = runs)
	uint32_t *front, *front_sum; // [n + 1] decal runs: the pair goes to the front part; exclusive sum
	uint32_t *run_start;   // [n + 1] first pair of run r; run_start[runs] = n
	uint32_t *run_bytes, *run_offset; // [n + 1] 16-byte aligned slice sizes (zero behind the last run), exclusive sum
	// outputs
	LmxDrawRun* runs;
	uint8_t* instance_data;
	uint8_t* group_data;
	uint32_t* counts;      // {runs, instance bytes, pairs, group records}
};
constexpr uint32_t DRAW_TILE = 256;
hipError_t launch_draw_flags(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v);   // flags + tile functions + tile scan + head flags
hipError_t launch_draw_runs(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v);    // (behind the sum of head) run starts, near-plane bits, slice sizes
hipError_t launch_draw_encode(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v);  // (behind the sums of front / run_bytes) run + instance records
hipError_t launch_draw_groups(hipStream_t s, const DrawDevice& d, const DrawViewDevice& v);  // the "fill instance data" block

// ---- PoseProcessor (pose_kernels.hip): the listed instances' dual quaternions packed into the frame's buffer, pose->slice by entity ----
// Frame state words. The first four are LmxPosesCounts; POSES_BYTES is the frame's cursor.
enum { POSES_INSTANCES = 0, POSES_BYTES = 1, POSES_SKIPPED = 2, POSES_OVERFLOW = 3, POSES_BASE = 4 /* the cursor the running pass started from */,
	POSES_LIST_N = 5 /* the length of a caller-given list */, POSES_STATE_WORDS = 8 };
constexpr uint32_t POSE_BONE_BYTES = 32;  // sizeof(DualQuat)
constexpr uint32_t POSE_BLOCK = 256;
constexpr uint32_t POSE_GRID = 256;       // blocks of the two slice steps: each owns a contiguous part of the list
constexpr uint32_t POSE_DQ_GRID = 1024;   // blocks of the dual-quaternion step: 4096 waves stride over the list's entries
struct PosesDevice {
	const int32_t* list;           // entities, in hand-over order
	const uint32_t* list_count;    // on the device: KEYS_N_POSES of the last key run, or POSES_LIST_N
	uint32_t list_cap;             // entries the list and `entries` hold (<= 2^31)
	const int32_t* skin_of_entity; uint32_t n_entities; // skin instance by entity, -1: none
	const SkinInstance* inst; uint32_t n_inst;
	const float* pose_pos; const float4* pose_rot;      // absolute poses (lmx_skin_run with pose write-back)
	const float* inv_pos; const float4* inv_rot;
	uint4* entries;                // [list_cap] {slice offset (in: entity), first pose bone, n_bones, first model bone}; y = 0xffffffff: no slice
	uint32_t* block_sum;           // [POSE_GRID]
	uint32_t* state;               // POSES_*
	float4* dual_quats; uint32_t cap_bytes;
	uint32_t handle, base_offset;
	uint32_t *bones_handle, *bones_offset; uint32_t n_table; // DrawDevice::bones_* (by entity)
};
hipError_t launch_pose_slices(hipStream_t s, const PosesDevice& d);     // sizes, offsets, slice tables, cursor and counters
hipError_t launch_pose_dual_quats(hipStream_t s, const PosesDevice& d); // (behind launch_pose_slices) the slices' contents

// ---- fillClusters (cluster_kernels.hip): light / probe records, per-cluster counts, offsets, the map ----
// State words = LmxClustersCounts.
enum { CLUSTERS_LIGHTS = 0, CLUSTERS_ENV = 1, CLUSTERS_REFL = 2, CLUSTERS_MAP = 3, CLUSTERS_OVERFLOW = 4, CLUSTERS_LIST_N = 5 /* the length of a caller-given list */,
	CLUSTERS_STATE_WORDS = 8 };
constexpr uint32_t CLUSTER_BLOCK = 256;        // threads per block of the record, count and fill steps; a light tile of the gather = one block's threads
constexpr uint32_t CLUSTER_REC_GRID = 256;     // blocks of the record step that stride over the list
constexpr uint32_t CLUSTER_PROBE_BLOCKS = 8;   // ... and the blocks behind them that take the probes (8 x 256 = one thread per probe of both kinds)
constexpr uint32_t CLUSTER_GRID = 1024;        // blocks of the count and fill steps: each wave owns a cluster, the blocks stride over the grid
constexpr uint32_t CLUSTER_SCAN_BLOCK = 1024;  // threads of the one block that sums the clusters' sizes
constexpr uint32_t CLUSTER_MAX_CLUSTERS = 64 * 64 * 16;
constexpr uint32_t CLUSTER_N_PLANES = 65 + 65 + 17; // x planes at 0, y planes at 65, z planes at 130
struct ClusterPlanesArg { float4 planes[CLUSTER_N_PLANES]; };
struct ClusterEnvRec { float4 v[13]; };  // ClusterEnvProbe, 208 B: {pos, pad0} {rot} {inner_range, pad1} {outer_range, pad2} sh_coefs[9]
struct ClusterReflRec { float4 v[3]; };  // ClusterReflProbe, 48 B: {pos, layer} {rot} {half_extents, pad1}
struct ClustersDevice {
	const int32_t* list;           // light entities, in list order
	const uint32_t* list_count;    // on the device: the cull result's LOCAL_LIGHT total, or CLUSTERS_LIST_N
	uint32_t list_cap;             // entries the list and `ranges` hold (<= 2^30)
	// World::getTransforms() as the draw pass reads it (lmx_entity_tr.h)
	const LmxTransform* tr; uint32_t n_tr;
	const double *wpx, *wpy, *wpz; const float4* wrot; const float *wsx, *wsy, *wsz; const int32_t* slot_of_entity; uint32_t n_world;
	const LmxPointLight* light_tab; uint32_t n_light_tab;
	const uint32_t* atlas; uint32_t n_atlas;          // nullptr: 0xffffffff for every entity
	// the enabled probes in output order: entity, radius (length of outer_range / half_extents) and the record with pos / rot left open
	const int32_t* env_entity; const float* env_radius; const ClusterEnvRec* env_tmpl; uint32_t n_env;
	const int32_t* refl_entity; const float* refl_radius; const ClusterReflRec* refl_tmpl; uint32_t n_refl;
	double cam[3];
	uint32_t size_x, size_y, size_z, n_clusters;
	uint32_t max_lights, map_capacity;
	// scratch: per listed light / per probe (env first) the cluster range {(x.lo + 1) | (x.hi + 1) << 8 | (y.lo + 1) << 16 | (y.hi + 1) << 24, the
	// same of z}: zero = in no cluster; the clusters' sizes and their exclusive sum
	uint2* ranges; uint2* probe_ranges;
	uint32_t *totals, *offsets;
	// outputs
	float4* lights;                // [max_lights] ClusterLight, 4 x float4
	int32_t* light_entities;       // [max_lights]
	uint4* clusters;               // [n_clusters] {offset, lights_count, env_probes_count, refl_probes_count}
	int32_t* map;                  // [map_capacity]
	ClusterEnvRec* env_out; ClusterReflRec* refl_out;
	uint32_t* state;               // CLUSTERS_*
};
hipError_t launch_cluster_records(hipStream_t s, const ClustersDevice& d, const ClusterPlanesArg& p); // light records + ranges, probe records + ranges
hipError_t launch_cluster_bins(hipStream_t s, const ClustersDevice& d);                                // (behind it) counts, offsets + counters, the map

// ---- castRay (ray_kernels.hip): rays x model instances -> candidates -> nearest triangle per candidate -> nearest entity per ray ----
// State words. The first three are LmxRaysCounts.
// The launch constants below are GUESSES: nothing has been measured yet; tools/ray_time.py is the tool to retune them with.
enum { RAYS_RAYS = 0, RAYS_CANDIDATES = 1, RAYS_OVERFLOW = 2, RAYS_COUNTER = 4 /* two words: the 64-bit append cursor of the broad phase (rays x entities can pass 2^32); RAYS_CANDIDATES is its value saturated at 2^32 - 1 */,
	RAYS_STATE_WORDS = 8 };
constexpr uint32_t RAY_BLOCK = 256;          // threads per block of every step
constexpr uint32_t RAY_BROAD_RAYS = 64;      // rays a block of the broad phase stages in LDS per tile; the tile's other side is one entity per thread
constexpr uint32_t RAY_BROAD_GRID = 2048;    // blocks of the broad phase: they stride over the (entity tile, ray tile) pairs
constexpr uint32_t RAY_RUN = 4;              // consecutive triangles per work item of the narrow phase
constexpr uint32_t RAY_NARROW_SPLIT = 4;     // blocks that share a candidate: block j of them takes the chunks j, j + 4, ... of RAY_BLOCK * RAY_RUN triangles
constexpr uint32_t RAY_NARROW_GRID = 4096;   // blocks of the narrow phase: RAY_NARROW_GRID / RAY_NARROW_SPLIT candidates at a time
constexpr uint32_t RAY_RESOLVE_GRID = 1024;  // blocks of the resolve and write-out steps: they stride over the candidates and the rays
constexpr uint32_t RAY_MAX_BONES = 256;      // Model::castRay's Matrix matrices[256]: a larger pose is cast unskinned
constexpr uint32_t RAY_NO_PALETTE = 0xffffffffu;
struct RayModelRec { float aabb_min[3], aabb_max[3]; float radius; uint32_t ready, first_mesh, n_meshes, n_tris /* of LOD 0 */, last_skinned /* the last LOD-0 mesh has a skin */, mesh_base /* index of the first LOD-0 mesh in the model's own mesh list */, pad; };
struct RayMeshRec { uint32_t first_tri /* ordinal of its first triangle in the model's LOD 0 */, n_tris, index_at /* bytes into `indices`, 4-byte aligned */, index_bytes /* 2 or 4 */, vert_at, n_verts, skin_at /* into `skins`, or 0xffffffff */, pad; };
// A pair that passed the broad phase: the model-space ray of the entity, its model and the first bone of its palette (RAY_NO_PALETTE: cast unskinned)
struct RayCandidate { uint32_t ray, entity; float o[3], d[3]; uint32_t model, palette_at, n_bones, pad; };
static_assert(sizeof(RayCandidate) == 48, "three 16-byte stores");
struct RaysDevice {
	const LmxRay* rays; uint32_t n_rays;
	// the model instances by entity: model (-1: none) and ModelInstance::flags
	const int32_t* inst_model; const uint8_t* inst_flags; uint32_t n_inst;
	// World::getTransforms() as the draw pass reads it (lmx_entity_tr.h)
	const LmxTransform* tr; uint32_t n_tr;
	const double *wpx, *wpy, *wpz; const float4* wrot; const float *wsx, *wsy, *wsz; const int32_t* slot_of_entity; uint32_t n_world;
	const RayModelRec* models; uint32_t n_models;
	const RayMeshRec* meshes;
	const float* positions;        // xyz per vertex, the meshes back to back
	const LmxSkin* skins;
	const uint8_t* indices;
	// pose: the skin instance of an entity (lmx_poses_set_instances), the instances and the palette lmx_skin_run left (nullptr: nobody is skinned)
	const int32_t* skin_of_entity; uint32_t n_skin_entities;
	const SkinInstance* skin_inst; uint32_t n_skin_inst;
	const float4* palette;         // 3 x float4 per bone (skin_kernels.hip "Palette layout")
	// scratch
	RayCandidate* cand; uint32_t max_cand;
	unsigned long long* cand_best; // [max_cand] (t bits << 32) | triangle ordinal, all ones: no hit
	float* cand_t;                 // [max_cand] new_t of a candidate with a hit
	unsigned long long* ray_best;  // [max_rays] (new_t bits << 32) | entity, all ones: no hit
	// outputs
	LmxRayHit* hits;
	uint32_t* state;               // RAYS_*
};
hipError_t launch_rays_broad(hipStream_t s, const RaysDevice& d);   // steps 1-6: the candidate list and its counters
hipError_t launch_rays_narrow(hipStream_t s, const RaysDevice& d);  // (behind it) Model::castRay per candidate
hipError_t launch_rays_resolve(hipStream_t s, const RaysDevice& d); // (behind it) world-space t per candidate, the minimum per ray, the hit records

// ---- castRayInstancedModels (ray_kernels.hip, k_imray_*): rays x instances of the attached instanced models, ahead of the stage above ----
// The stage has state words of its own in the RAYS_* layout (k_ray_narrow reads its cursor there): the first three are LmxRaysImCounts.
// Word RAYS_IM_OVERFLOW of the ENTITY stage's state carries this stage's overflow (0 or 2) into LmxRaysCounts::overflow.
// The launch constants below are GUESSES as well: none has been compared on a GPU; tools/ray_im_time.py is the tool.
enum { RAYS_IM_OVERFLOW = 3 };
constexpr uint32_t RAY_IM_BROAD_GRID = 2048; // blocks of k_imray_broad: they stride over the (256-slot instance tile, ray tile) pairs
struct RayImModelRec { int32_t ray_model /* of lmx_rays_set_models, -1: none */, entity; };
struct ImRaysDevice {
	RaysDevice r;                  // the shared tables and scratch; rays = the caller's, state = the stage's own words, hits unused
	// the attached LmxInstancedModels (lmx_im.h): ImModelDev table, model of every IM_TILE tile, the instances in grid order
	const struct ImModelDev* im_models; uint32_t n_im_models;
	const uint32_t* tile_model; uint32_t n_tiles;
	const float4* pos_scale; const float4* rot;
	const RayImModelRec* im_ray_models; // [n_im_models]
	unsigned long long* im_best;   // [max_rays] (ordered bits of t_model * scale << 32) | global slot, all ones: no hit
	LmxRayImHit* im_hits;          // [max_rays]
	LmxRay* rays_eff;              // [max_rays] the rays with the effective t_max: what the entity stage casts
	uint32_t* entity_state;        // the entity stage's RAYS_* words (RAYS_IM_OVERFLOW)
};
hipError_t launch_imrays_broad(hipStream_t s, const ImRaysDevice& d);   // the candidate list of (ray, instance) pairs and its cursor
hipError_t launch_imrays_resolve(hipStream_t s, const ImRaysDevice& d); // (behind launch_rays_narrow(d.r)) t_model * scale, the minimum per ray, hit records, effective rays, counters

// ---- castRayProceduralGeometry, Terrain::castRay and castRay's merge (ray_scene_kernels.hip), behind the two stages above ----
// The procedural stage has state words of its own in the RAYS_* layout (k_ray_narrow reads its cursor there): the first three are
// LmxRaysSceneCounts. Its overflow goes into the ENTITY stage's RAYS_OVERFLOW word as RAYS_PG_OVERFLOW (k_pgray_write runs behind k_ray_write).
// The launch constants below are GUESSES as well: none has been compared on a GPU; tools/ray_scene_time.py is the tool.
enum { RAYS_PG_OVERFLOW = 4 };
constexpr uint32_t RAY_PG_BROAD_GRID = 1024;  // blocks of k_pgray_broad: they stride over the (256-geometry tile, ray tile) pairs
constexpr uint32_t RAY_TERRAIN_CHUNK = 64;    // steps of a terrain walk a wave takes at a time: one cell per lane
constexpr uint32_t RAY_TERRAIN_GRID = 2048;   // blocks of k_terrain_ray: RAY_BLOCK / 64 (ray, terrain) pairs each, strided
constexpr uint32_t RAY_MAX_TERRAINS = 1024;   // entries of the terrain table (a batch holds rays x terrains hit records)
struct RayPgRec { int32_t entity; uint32_t castable /* has vertex data and is a triangle list */; };
struct RayTerrainRec { int32_t entity; uint32_t width, height, format /* LMX_RAY_TERRAIN_* */; float scale[3]; uint32_t ready; uint64_t texel_at /* bytes into `texels`, 4-byte aligned */; };
struct SceneRaysDevice {
	RaysDevice r;                  // rays = the caller's, the transforms, the shared scratch; models / meshes / positions / indices = the procedural
	                               // geometries' own tables (model g = geometry g, one mesh each); state = the stage's own words; hits unused
	const RayPgRec* pg; uint32_t n_pg;
	unsigned long long* pg_best;   // [max_rays] (ordered bits of t << 32) | geometry, all ones: no hit
	LmxRayPgHit* pg_hits;          // [max_rays]
	const RayTerrainRec* terrains; uint32_t n_terrains;
	const uint8_t* texels;         // the heightmaps as they were given, back to back
	LmxRayTerrainHit* terrain_hits; // [max_rays * n_terrains], ray-major
	const LmxRayHit* hits;         // the entity stage's
	const LmxRayImHit* im_hits;    // the instanced-model stage's, nullptr without one
	LmxRaySceneHit* scene_hits;    // [max_rays]
	uint32_t* entity_state;        // the entity stage's RAYS_* words (RAYS_OVERFLOW)
};
hipError_t launch_pgrays_broad(hipStream_t s, const SceneRaysDevice& d);   // the candidate list of (ray, geometry) pairs and its cursor
hipError_t launch_pgrays_resolve(hipStream_t s, const SceneRaysDevice& d); // (behind launch_rays_narrow(d.r)) the minimum per ray, LmxRayPgHit, counters
hipError_t launch_terrain_rays(hipStream_t s, const SceneRaysDevice& d);   // LmxRayTerrainHit per (ray, terrain)
hipError_t launch_scene_write(hipStream_t s, const SceneRaysDevice& d);    // (behind every stage) LmxRaySceneHit per ray

// Pose::computeAbsolute + computeSkinMatrices (+ optional dual-quaternion palette), one wave per PoseGroup
hipError_t launch_pose_palette(hipStream_t s, const SkinInstance* inst, const PoseGroup* groups, const uint32_t n_groups[3] /* by capacity 4, 2, 1 */,
	const float* rel_pos, const float4* rel_rot, float* pose_pos, float4* pose_rot, const uint32_t* level_items, const uint16_t* level_off,
	const float* inv_pos, const float4* inv_rot, float4* palette, float4* dual_quats /* optional */);
// Pose::blend over all bones of all instances
hipError_t launch_pose_blend(hipStream_t s, float* pos, float4* rot, const float* rhs_pos, const float4* rhs_rot, size_t n_bones, float weight);
// palette rows (3 x float4 per bone) -> column-major 4 x 4 matrices
hipError_t launch_palette_expand(hipStream_t s, const float4* rows, uint32_t n_bones, float4* out);
// evaluateSkin over every vertex of every instance
hipError_t launch_skin_vertices(hipStream_t s, const SkinInstance* inst, const uint32_t* inst_index /* optional subset */, uint32_t n_inst,
	uint32_t max_verts, const float4* mesh /* 2 x float4 per vertex: weights | (position, 4 x u8 bone indices) */,
	const float4* palette /* 3 rows per bone, or the dual quaternions in LMX_SKIN_DQS */, float* out, int mode);
// the same for runs of consecutive instances that share a mesh and a bone count (vertex records held in registers)
hipError_t launch_skin_shared(hipStream_t s, const SkinInstance* inst, const SkinChunk* chunks, uint32_t n_chunks, const float4* mesh_local,
	const uint8_t* tile_bones, const float4* palette, float* out, int mode);
// k_skin_multi: `per_block` instances per block (1, 2, 4, 8, 16; capped by skin_multi_instances for models above 64 bones). A work item
// carries everything the block needs (ONE dependent load at block start, not chunk -> instance -> palette): `count` consecutive
// instances of one model and one mesh - their palettes start at bone `bone_offset` (n_bones each), their outputs at vertex `out_offset`
// (n_verts each) - and the vertex range [v_begin, v_end) of the mesh whose first record in `mesh` (global bone indices) is rec_offset.
struct SkinMultiChunk { uint32_t bone_offset, n_bones, count, v_begin, v_end, rec_offset, n_verts, out_offset, n_stage /* bones staged in LDS: the mesh's largest bone index + 1 */; };
uint32_t skin_multi_instances(uint32_t per_block, uint32_t n_bones);
uint32_t skin_multi_lds_slots(uint32_t n_stage);
hipError_t launch_skin_multi(hipStream_t s, uint32_t per_block, const SkinMultiChunk* chunks, uint32_t n_chunks, uint32_t lds_slots /* largest skin_multi_lds_slots(n_stage) of the chunks */, const float4* mesh, const float4* palette, float* out, int mode);
constexpr uint32_t SKIN_SHARED_TILE_VERTS = 5120; // k_skin_shared: 1024 lanes x 5 vertex records

} // namespace lmx
