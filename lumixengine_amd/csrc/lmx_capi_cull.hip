// lmx_capi_cull.hip — CullingSystem behind the C ABI (include/lumix_mi355.h, "culling" section).
//
// Two resident sets, one visibility function:
//   * static set   host mirror of (cell, cell-relative sphere) per entity + a device layout sorted by (type, is_big, cell)
//                  with chunk headers and tile-major cell keys (lmx_cull_layout.h), culled by k_cull_tile. Between two
//                  compactions the layout only takes O(1) patches: an in-cell move rewrites 16 B, a removal turns the id
//                  into a tombstone (-1), and an entity that is added or leaves its cell goes to the dynamic set.
//   * dynamic set  unsorted world position (fp64) + radius per entity: entities bound to the world hierarchy
//                  (lmx_world_bind_culling, refreshed on the device by lmx_world_propagate) and the overflow of the static
//                  set. k_cull_dynamic re-derives cell, cell-relative position and per-cell class per entity — what
//                  CullingSystem::set + cullInternal would compute (culling_system.cpp:225-242, 321-369). Slots are
//                  stable: add takes a free slot, remove frees one, both cost one 40-byte patch.
// A compaction (structure rebuild) folds the unbound part of the dynamic set back into the sorted layout once it outgrows a
// threshold; it is the only operation that costs O(n).
// Both kernels write to per-shard output windows (see CullOut); k_cull_finalize / k_cull_consolidate turn those into per-type
// totals and contiguous lists on demand.
//
// The culling host layer is four translation units that share lmx_cull_host.h:
//   lmx_capi_cull_set.hip      the host mirror of the two sets, its O(1) mutations, add / remove / set* and their batched forms
//   lmx_capi_cull_async.hip    the asynchronous compaction (LMX_CULL_OPT_ASYNC_COMPACTION): shadow set, operation log, worker, swap
//   lmx_capi_cull.hip          (this file) patches, rebuilds, output layout, flush, build, the launch, options and stats
//   lmx_capi_cull_results.hip  totals, contiguous lists, host reads, the map protocol, view slots, bound outputs
#include "lmx_cull_host.h"

#include <optional>

using namespace lmx;

namespace {

static_assert(sizeof(LayoutSphere) == sizeof(float4) && sizeof(LayoutCell) == sizeof(CellKey) && sizeof(LayoutChunkHdr) == sizeof(ChunkHdr), "layout PODs mirror the device types");
static_assert(LAYOUT_MAX_TYPES == MAX_TYPES && LAYOUT_CHUNK == CHUNK && LAYOUT_TILE_ALIGN == TILE_ALIGN && LAYOUT_CELL_DEAD == CELL_DEAD, "layout constants");

constexpr uint32_t DYN_ALIGN = 2048;       // largest k_cull_dynamic tile: a tile never straddles two types
constexpr uint32_t DYN_MAX_SHARDS = 8;     // output shards per type of the dynamic set

CullDeviceView static_view(const CullSet& cs) {
	CullDeviceView v;
	v.spheres = cs.spheres.p;
	v.ids = cs.ids.p;
	v.hdr = cs.hdr.p;
	v.n_padded = cs.n_padded;
	v.keys_packed = cs.keys_packed;
	for (int k = 0; k < 3; ++k) {
		v.tile_cells[k] = cs.tile_cells[k].p;
		v.tile_tab[k] = cs.tile_tab[k].p;
		v.tile_box[k] = cs.tile_box[k].p;
		v.tile_cap[k] = cs.tile_cap[k];
		v.tile_out[k] = nullptr; // (belongs to the output layout: the caller fills it)
	}
	return v;
}

} // namespace

namespace lmx {

// Ship the queued patch records: one copy into pinned, device-visible host memory and ONE kernel that reads the records from there
// (a frame's records are tens of KB; the H2D copy call alone cost more host time than the 2000 mirror updates it carried) - no host
// wait: the two staging halves alternate, a half is rewritten two flushes after the kernel that read it was enqueued.
int apply_patches_on(LmxContext* ctx, CullSet& cs, hipStream_t stream, bool profile) {
	const size_t n_ps = cs.q_sphere.size(), n_pi = cs.q_id.size(), n_pd = cs.q_dyn.size();
	if (!(n_ps + n_pi + n_pd)) return LMX_OK;
	const size_t b_ps = n_ps * sizeof(PatchSphere), b_pi = n_pi * sizeof(PatchId), b_pd = n_pd * sizeof(PatchDyn);
	const size_t o_pd = 0, o_ps = (o_pd + b_pd + 15) & ~(size_t)15, o_pi = (o_ps + b_ps + 15) & ~(size_t)15; // PatchDyn needs 8-byte alignment
	const size_t total = o_pi + b_pi;
	PatchStaging& st = cs.staging;
	const uint32_t k = st.next;
	st.next ^= 1u;
	if (!st.done[k]) LMX_HIP(ctx, hipEventCreateWithFlags(&st.done[k], hipEventDisableTiming));
	else LMX_HIP(ctx, hipEventSynchronize(st.done[k])); // the kernel that last read this half (two flushes ago) has long finished
	if (st.cap[k] < total) {
		if (st.host[k]) LMX_HIP(ctx, hipHostFree(st.host[k]));
		st.host[k] = nullptr;
		st.dev[k] = nullptr;
		st.cap[k] = 0;
		const size_t want = std::max<size_t>(total * 2, 1u << 16);
		LMX_HIP(ctx, hipHostMalloc(&st.host[k], want, hipHostMallocMapped));
		LMX_HIP(ctx, hipHostGetDevicePointer(&st.dev[k], st.host[k], 0));
		st.cap[k] = want;
	}
	char* h = (char*)st.host[k];
	if (b_pd) memcpy(h + o_pd, cs.q_dyn.data(), b_pd);
	if (b_ps) memcpy(h + o_ps, cs.q_sphere.data(), b_ps);
	if (b_pi) memcpy(h + o_pi, cs.q_id.data(), b_pi);
	const char* d = (const char*)st.dev[k];
	TileBox* const boxes[3] = {cs.tile_box[0].p, cs.tile_box[1].p, cs.tile_box[2].p};
	if (&cs == static_cast<CullSet*>(&ctx->cull) && n_pi) { // a slot about to become a tombstone: its per-slot sort-key state follows the entity
		if (int rc = keys_before_tombstones(ctx, (const PatchId*)(d + o_pi), (uint32_t)n_pi)) return rc;
	}
	{
		std::optional<ProfScope> ps; // (the profiler's event pool belongs to the update thread: the worker of the asynchronous compaction passes false)
		if (profile) ps.emplace(ctx, LMX_K_CULL_PATCH);
		LMX_HIP(ctx, launch_apply_patches(stream, cs.spheres.p, cs.ids.p, boxes, dyn_view(cs), (const PatchSphere*)(d + o_ps), (uint32_t)n_ps,
			(const PatchId*)(d + o_pi), (uint32_t)n_pi, (const PatchDyn*)(d + o_pd), (uint32_t)n_pd));
	}
	LMX_HIP(ctx, hipEventRecord(st.done[k], stream));
	clear_static_queues(cs);
	clear_dyn_queue(cs);
	return LMX_OK;
}

// Rebuild the static device layout from the host mirror (lmx_cull_layout.h) and upload it.
int rebuild_static_on(LmxContext* ctx, CullSet& cs, hipStream_t stream, uint32_t overflow_reserve, PinnedUploader* up) {
	CullLayout lay;
	if (!build_cull_layout(cs.recs, lay)) return fail(ctx, LMX_ERR_CAPACITY, "too many spheres (%zu)", cs.recs.size());
	const size_t n_padded = lay.n_padded;
	const size_t n_chunks = n_padded / CHUNK;
	double scene_lo[3], scene_hi[3];
	for (int a = 0; a < 3; ++a) { scene_lo[a] = INFINITY; scene_hi[a] = -INFINITY; }
	size_t big_tiles = 0, live_tiles = 0;
	for (const TileBox& b : lay.tile_box[0]) { // world-space box of the occupied cells (static set)
		if (b.flags & TILE_EMPTY) continue;
		++live_tiles;
		if (b.flags & TILE_HAS_BIG) ++big_tiles;
		for (int a = 0; a < 3; ++a) {
			scene_lo[a] = std::min(scene_lo[a], (double)CELL_SIZE * b.lo[a]);
			scene_hi[a] = std::max(scene_hi[a], (double)CELL_SIZE * b.hi[a] + (double)CELL_SIZE);
		}
	}
	// the buffers below may be reallocated; the copies are ordered on `stream` - the context's for the synchronous path, the worker's own
	// for the asynchronous compaction (a plain hipMemcpy would go through the null stream and order itself against every blocking stream)
	LMX_HIP(ctx, hipStreamSynchronize(stream));
	// From here to the commit at the end the device buffers hold neither layout for certain (a reserve may have replaced one, an upload may
	// have failed half way): every early return leaves the set as "not built, rebuild due", with the metadata of the older layout untouched
	// and unread - no cull can run before a later flush has rebuilt and committed.
	cs.built = false;
	cs.structure_dirty = true;
	LMX_HIP(ctx, cs.spheres.reserve(std::max<size_t>(n_padded, 1)));
	LMX_HIP(ctx, cs.ids.reserve(std::max<size_t>(n_padded, 1)));
	LMX_HIP(ctx, cs.hdr.reserve(std::max<size_t>(n_chunks, 1)));
	if (n_padded) {
		LMX_HIP(ctx, upload_via(up, cs.spheres.p, lay.spheres.data(), n_padded * sizeof(float4), stream));
		LMX_HIP(ctx, upload_via(up, cs.ids.p, lay.ids.data(), n_padded * sizeof(int32_t), stream));
		LMX_HIP(ctx, upload_via(up, cs.hdr.p, lay.hdr.data(), n_chunks * sizeof(ChunkHdr), stream));
	}
	// Cell keys travel in 8 bytes where every tile's cells lie within 65535 cell indices of its box's low corner (any scene that is not a handful
	// of entities millions of units apart): offsets against TileBox::lo + the two flags the kernel reads (PackedCellKey). 4096-sphere tiles (k = 0)
	// are walked by no kernel since round 6: their keys are not uploaded at all (their boxes are: k_apply_patches clears TILE_DENSE in all three).
	bool packable = getenv("LMX_CULL_WIDE_KEYS") == nullptr;
	for (int k = 1; k < 3 && packable; ++k) {
		for (size_t ti = 0; ti < lay.tile_box[k].size() && packable; ++ti) {
			const TileBox& b = lay.tile_box[k][ti];
			if (b.flags & TILE_EMPTY) continue;
			for (int a = 0; a < 3; ++a) packable = packable && (int64_t)b.hi[a] - (int64_t)b.lo[a] <= 65535;
		}
	}
	std::vector<PackedCellKey> packed_k[3]; // (alive until the synchronize below: the copies are asynchronous)
	for (int k = 0; k < 3; ++k) {
		const bool keys_used = k != 0;
		const size_t key_bytes = !keys_used ? 0 : lay.tile_cells[k].size() * (packable ? sizeof(PackedCellKey) : sizeof(CellKey));
		LMX_HIP(ctx, cs.tile_cells[k].reserve(std::max<size_t>((key_bytes + sizeof(CellKey) - 1) / sizeof(CellKey), 1)));
		LMX_HIP(ctx, cs.tile_tab[k].reserve(std::max<size_t>(lay.tile_tab[k].size(), 1)));
		LMX_HIP(ctx, cs.tile_box[k].reserve(std::max<size_t>(lay.tile_box[k].size(), 1)));
		if (!lay.tile_cells[k].empty()) {
			if (keys_used && packable) {
				const size_t cap = lay.tile_cap[k];
				std::vector<PackedCellKey>& packed = packed_k[k];
				packed.resize(lay.tile_cells[k].size());
				parallel_ranges(lay.tile_box[k].size(), [&](size_t tb, size_t te) {
					for (size_t ti = tb; ti < te; ++ti) {
						const TileBox& b = lay.tile_box[k][ti];
						for (size_t j = 0; j < cap; ++j) {
							const LayoutCell& c = lay.tile_cells[k][ti * cap + j];
							PackedCellKey pk{0u, PACKED_CELL_DEAD};
							if (!(c.meta & LAYOUT_CELL_DEAD))
								pk = PackedCellKey{(uint32_t)(c.ix - b.lo[0]) | ((uint32_t)(c.iy - b.lo[1]) << 16), (uint32_t)(c.iz - b.lo[2]) | ((c.meta & 0x100u) ? PACKED_CELL_BIG : 0u)};
							packed[ti * cap + j] = pk;
						}
					}
				});
				LMX_HIP(ctx, upload_via(up, cs.tile_cells[k].p, packed.data(), key_bytes, stream));
			} else if (keys_used) {
				LMX_HIP(ctx, upload_via(up, cs.tile_cells[k].p, lay.tile_cells[k].data(), key_bytes, stream));
			}
			LMX_HIP(ctx, upload_via(up, cs.tile_tab[k].p, lay.tile_tab[k].data(), lay.tile_tab[k].size() * sizeof(uint32_t), stream));
			LMX_HIP(ctx, upload_via(up, cs.tile_box[k].p, lay.tile_box[k].data(), lay.tile_box[k].size() * sizeof(TileBox), stream));
		}
	}
	LMX_HIP(ctx, hipStreamSynchronize(stream)); // `lay` is about to go
	// commit: the device holds the new layout, the set describes it
	for (int t = 0; t < MAX_TYPES; ++t) {
		cs.tt.ent_start[t] = lay.ent_start[t];
		cs.tt.ent_end[t] = lay.ent_end[t];
	}
	cs.n_padded = (uint32_t)n_padded;
	cs.n_cells = (uint32_t)lay.cells.size();
	cs.n_dead_cells = lay.n_dead_cells;
	for (int k = 0; k < 3; ++k) {
		cs.max_tile_cells[k] = lay.max_tile_cells[k];
		cs.tile_cap[k] = lay.tile_cap[k];
		cs.scene_lo[k] = scene_lo[k];
		cs.scene_hi[k] = scene_hi[k];
	}
	cs.big_tile_fraction = live_tiles ? (double)big_tiles / (double)live_tiles : 0.0;
	cs.keys_packed = packable;
	cs.rec_slot.swap(lay.rec_slot);
	cs.block_live.swap(lay.block_live);
	cs.structure_dirty = false;
	cs.built = true;
	if (overflow_reserve) cs.dyn_layout_dirty = true; // the reserve follows the new static set's type shares
	cs.n_tombstones = 0;
	clear_static_queues(cs);
	return LMX_OK;
}
std::atomic<uint64_t> g_layout_generation{1};
static int rebuild_static(LmxContext* ctx) {
	if (int rc = keys_before_layout_change(ctx)) return rc; // per-slot state of the sort-key tables goes back to its entity-indexed home first
	if (int rc = rebuild_static_on(ctx, ctx->cull, ctx->stream, ctx->cull.overflow_reserve)) return rc;
	ctx->cull.layout_generation = g_layout_generation++;
	return LMX_OK;
}

// (Re)assign the device slots of the dynamic set: one region per type, padded to DYN_ALIGN, with room to grow
// (region = 1.5 x live + one tile), and upload everything.
int rebuild_dynamic_on(LmxContext* ctx, CullSet& cs, hipStream_t stream, uint32_t overflow_reserve, PinnedUploader* up) {
	const size_t n = cs.dyn.size();
	size_t count_by_type[MAX_TYPES] = {};
	for (const DynRec& r : cs.dyn) count_by_type[r.type]++;
	// LMX_CULL_OPT_OVERFLOW_RESERVE: room for that many more entities, shared out over the renderable types by their share of the
	// static set, so that adds / re-celling sets between compactions take free slots and never trigger this function again
	size_t static_by_type[MAX_TYPES] = {}, static_total = 0;
	for (int t = 0; t < MAX_TYPES; ++t) {
		static_by_type[t] = cs.tt.ent_end[t] - cs.tt.ent_start[t];
		static_total += static_by_type[t];
	}
	size_t padded = 0;
	for (int t = 0; t < MAX_TYPES; ++t) {
		cs.dyn_tt.ent_start[t] = (uint32_t)padded;
		size_t want = count_by_type[t] ? count_by_type[t] + count_by_type[t] / 2 + DYN_ALIGN : 0;
		if (overflow_reserve && static_by_type[t]) want = std::max<size_t>(want, count_by_type[t] + (size_t)((double)overflow_reserve * static_by_type[t] / static_total) + DYN_ALIGN);
		if (want) padded += want / DYN_ALIGN * DYN_ALIGN;
		cs.dyn_tt.ent_end[t] = (uint32_t)padded;
		cs.dyn_free[t].clear();
	}
	if (padded > 0x7fffffffull) return fail(ctx, LMX_ERR_CAPACITY, "too many dynamic spheres (%zu)", n);
	std::vector<double> px(padded, 0.0), py(padded, 0.0), pz(padded, 0.0);
	std::vector<float> radius(padded, 0.f);
	std::vector<int32_t> ids(padded, -1);
	size_t cursor[MAX_TYPES];
	for (int t = 0; t < MAX_TYPES; ++t) cursor[t] = cs.dyn_tt.ent_start[t];
	for (size_t i = 0; i < n; ++i) {
		DynRec& r = cs.dyn[i];
		const size_t s = cursor[r.type]++;
		r.slot = (uint32_t)s;
		px[s] = r.pos[0];
		py[s] = r.pos[1];
		pz[s] = r.pos[2];
		radius[s] = r.radius;
		ids[s] = r.entity;
	}
	for (int t = 0; t < MAX_TYPES; ++t) cs.dyn_next[t] = (uint32_t)cursor[t];
	cs.dyn_padded = (uint32_t)padded;
	const size_t cap = std::max<size_t>(padded, 1);
	LMX_HIP(ctx, hipStreamSynchronize(stream));
	LMX_HIP(ctx, cs.dyn_px.reserve(cap));
	LMX_HIP(ctx, cs.dyn_py.reserve(cap));
	LMX_HIP(ctx, cs.dyn_pz.reserve(cap));
	LMX_HIP(ctx, cs.dyn_radius.reserve(cap));
	LMX_HIP(ctx, cs.dyn_ids.reserve(cap));
	if (padded) {
		LMX_HIP(ctx, upload_via(up, cs.dyn_px.p, px.data(), padded * sizeof(double), stream));
		LMX_HIP(ctx, upload_via(up, cs.dyn_py.p, py.data(), padded * sizeof(double), stream));
		LMX_HIP(ctx, upload_via(up, cs.dyn_pz.p, pz.data(), padded * sizeof(double), stream));
		LMX_HIP(ctx, upload_via(up, cs.dyn_radius.p, radius.data(), padded * sizeof(float), stream));
		LMX_HIP(ctx, upload_via(up, cs.dyn_ids.p, ids.data(), padded * sizeof(int32_t), stream));
		LMX_HIP(ctx, hipStreamSynchronize(stream)); // the staging vectors are about to go
	}
	cs.dyn_layout_dirty = false;
	cs.q_dyn.clear();
	cs.q_dyn_at.assign(padded, ~0u);
	cs.dyn_generation++;
	return LMX_OK;
}

// Output shards: per type, the windows of the static set's shards, then those of the dynamic set's. A static window holds
// exactly the live ids of its blocks; a dynamic window the slots of its tiles.
int recompute_out_layout(LmxContext* ctx) {
	CullState& cs = ctx->cull;
	cs.shard_type.clear();
	cs.win_base.clear();
	uint32_t off = 0, max_cap = 0;
	for (int t = 0; t < MAX_TYPES; ++t) {
		cs.type_start[t] = off;
		const uint32_t s_blocks = (cs.tt.ent_end[t] - cs.tt.ent_start[t]) / TILE_ALIGN;
		const uint32_t s_n = std::min(s_blocks, std::max(1u, cs.max_shards));
		cs.tt.shard_first[t] = (uint32_t)cs.win_base.size();
		cs.tt.shard_n[t] = s_n;
		if (s_n) {
			std::vector<uint32_t> cap(s_n, 0u);
			const uint32_t b0 = cs.tt.ent_start[t] / TILE_ALIGN;
			for (uint32_t b = 0; b < s_blocks; ++b) cap[b % s_n] += cs.block_live[b0 + b];
			for (uint32_t k = 0; k < s_n; ++k) {
				cs.win_base.push_back(off);
				cs.shard_type.push_back((uint8_t)t);
				off += cap[k];
				max_cap = std::max(max_cap, cap[k]);
			}
		}
		const uint32_t d_blocks = (cs.dyn_tt.ent_end[t] - cs.dyn_tt.ent_start[t]) / DYN_ALIGN;
		const uint32_t d_n = std::min(d_blocks, DYN_MAX_SHARDS);
		cs.dyn_tt.shard_first[t] = (uint32_t)cs.win_base.size();
		cs.dyn_tt.shard_n[t] = d_n;
		for (uint32_t k = 0; k < d_n; ++k) {
			const uint32_t cap = ((d_blocks - k + d_n - 1) / d_n) * DYN_ALIGN; // blocks k, k + d_n, ...
			cs.win_base.push_back(off);
			cs.shard_type.push_back((uint8_t)t);
			off += cap;
			max_cap = std::max(max_cap, cap);
		}
		cs.type_cap[t] = off - cs.type_start[t];
	}
	cs.out_total = off;
	cs.n_shards = (uint32_t)cs.win_base.size();
	cs.max_shard_cap = max_cap;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, cs.d_win_base.reserve(std::max<size_t>(cs.n_shards, 1)));
	LMX_HIP(ctx, cs.d_shard_type.reserve(std::max<size_t>(cs.n_shards, 1)));
	LMX_HIP(ctx, cs.d_type_start.reserve(MAX_TYPES));
	LMX_HIP(ctx, upload_blocking(cs.d_win_base.p, cs.win_base));
	LMX_HIP(ctx, upload_blocking(cs.d_shard_type.p, cs.shard_type));
	LMX_HIP(ctx, upload_blocking(cs.d_type_start.p, cs.type_start, MAX_TYPES));
	for (int k = 0; k < 3; ++k) { // every tile's shard and window start, per tile size (k_cull_tile reads one 8-byte entry instead of deriving them)
		const uint32_t tile = TILE_ALIGN >> k;
		std::vector<uint2> tab(cs.n_padded / tile);
		for (int t = 0; t < MAX_TYPES; ++t) {
			for (uint32_t e = cs.tt.ent_start[t]; e < cs.tt.ent_end[t]; e += tile) {
				const uint32_t shard = cs.tt.shard_first[t] + ((e - cs.tt.ent_start[t]) / TILE_ALIGN) % cs.tt.shard_n[t];
				tab[e / tile] = make_uint2(shard, cs.win_base[shard]);
			}
		}
		LMX_HIP(ctx, upload_blocking(cs.d_tile_out[k], tab));
	}
	for (CullView& v : cs.views) {
		v.valid = v.finalized = v.consolidated = false;
		v.cnt_words = 0; // counters are re-sized (and zeroed) by the next cull on the view
	}
	return LMX_OK;
}

bool wants_compaction(const CullState& cs) {
	if (!layout_live(cs)) return true;
	if (!cs.auto_compaction) return false; // the host schedules lmx_cull_compact itself (loading screen, level streaming boundary)
	const size_t n_static = cs.recs.size();
	return cs.n_unbound > std::max<size_t>(cs.compaction_min, n_static / 8) || cs.n_tombstones > std::max<size_t>(cs.compaction_min, n_static / 4);
}

static int flush_impl(LmxContext* ctx, bool force_compaction) {
	CullState& cs = ctx->cull;
	bool layout_changed = false;
	bool compact = wants_compaction(cs) || (force_compaction && (cs.n_unbound || cs.n_tombstones));
	if (cs.async && layout_live(cs) && !force_compaction) {
		// the re-sort belongs to the worker: hand it this flush's operations, adopt its result if one is ready, ask for a job when due
		bool swapped = false;
		if (int rc = async_poll(ctx, &swapped)) return rc;
		compact = false;
		(void)swapped; // (async_swap re-derived the output layout itself)
	}
	if (compact && cs.async) async_wait_idle(*cs.async); // a synchronous rebuild (first build, lmx_cull_compact): the shadow set is re-seeded below
	if (compact) {
		if (cs.built && cs.n_unbound) {
			cs.structure_dirty = true; // from here on the mirror ops below must not queue patches against the old layout
			fold_overflow(cs);
		}
		cs.structure_dirty = true;
		if (int rc = rebuild_static(ctx)) return rc;
		layout_changed = true;
		if (cs.async) async_reseed(cs); // the live set changed outside the operation log
	}
	if (cs.dyn_layout_dirty) {
		if (int rc = cull_dyn_sync_mirror(ctx)) return rc; // keep what the device refreshed before slots move
		if (int rc = rebuild_dynamic_on(ctx, cs, ctx->stream, cs.overflow_reserve)) return rc;
		layout_changed = true;
	}
	if (layout_changed) {
		if (int rc = recompute_out_layout(ctx)) return rc;
	}
	return apply_patches_on(ctx, cs, ctx->stream, true);
}

// dyn[] <- device for the entities lmx_world_propagate refreshes (the host is the only writer of everything else)
int cull_dyn_sync_mirror(LmxContext* ctx) {
	CullState& cs = ctx->cull;
	if (!cs.dyn_mirror_stale) return LMX_OK;
	cs.dyn_mirror_stale = false;
	if (!cs.dyn_padded) return LMX_OK;
	LMX_CHECK_CTX(ctx); // reached from host-only entry points too
	if (int rc = apply_patches_on(ctx, cs, ctx->stream, true)) return rc; // host-side sets queued since the refresh are newer than what the device holds
	const size_t padded = cs.dyn_padded;
	std::vector<double> px(padded), py(padded), pz(padded);
	std::vector<float> radius(padded);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, hipMemcpy(px.data(), cs.dyn_px.p, padded * sizeof(double), hipMemcpyDeviceToHost));
	LMX_HIP(ctx, hipMemcpy(py.data(), cs.dyn_py.p, padded * sizeof(double), hipMemcpyDeviceToHost));
	LMX_HIP(ctx, hipMemcpy(pz.data(), cs.dyn_pz.p, padded * sizeof(double), hipMemcpyDeviceToHost));
	LMX_HIP(ctx, hipMemcpy(radius.data(), cs.dyn_radius.p, padded * sizeof(float), hipMemcpyDeviceToHost));
	for (DynRec& r : cs.dyn) {
		if (!r.bound || r.slot == DYN_NO_SLOT || r.slot >= padded) continue;
		r.pos[0] = px[r.slot];
		r.pos[1] = py[r.slot];
		r.pos[2] = pz[r.slot];
		r.radius = radius[r.slot];
	}
	return LMX_OK;
}

int cull_flush(LmxContext* ctx) { return flush_impl(ctx, false); }

} // namespace lmx

extern "C" {

int lmx_cull_build(LmxContext* ctx, uint32_t n, const int32_t* entity, const uint8_t* type, const double* pos_xyz, const float* radius) {
	LMX_CHECK_CTX(ctx);
	if (n && (!entity || !type || !pos_xyz || !radius)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null input array");
	CullState& cs = ctx->cull;
	int32_t max_entity = -1;
	for (uint32_t i = 0; i < n; ++i) {
		if (entity[i] < 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity[%u] = %d is negative", i, entity[i]);
		if (type[i] >= MAX_TYPES) return fail(ctx, LMX_ERR_CAPACITY, "type[%u] = %u >= LMX_MAX_TYPES", i, type[i]);
		max_entity = std::max(max_entity, entity[i]);
	}
	cs.recs.clear();
	cs.dyn.clear();
	cs.ent_to_dyn.clear();
	cs.n_unbound = 0;
	cs.dyn_layout_dirty = true;
	cs.dyn_mirror_stale = false;
	clear_static_queues(cs);
	cs.q_dyn.clear();
	cs.q_dyn_at.clear();
	cs.ent_to_rec.assign((size_t)max_entity + 1, -1);
	cs.structure_dirty = true;
	for (uint32_t i = 0; i < n; ++i) {
		if (cs.ent_to_rec[entity[i]] >= 0) {
			cs.recs.clear();
			cs.ent_to_rec.clear();
			return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "entity %d added twice", entity[i]);
		}
		cs.ent_to_rec[entity[i]] = (int32_t)i;
	}
	cs.recs.resize(n);
	parallel_ranges(n, [&](size_t b, size_t e) {
		for (size_t i = b; i < e; ++i) cs.recs[i] = make_cull_rec(entity[i], type[i], DV3{pos_xyz[3 * i], pos_xyz[3 * i + 1], pos_xyz[3 * i + 2]}, radius[i]);
	});
	return cull_flush(ctx);
}

int lmx_cull_flush(LmxContext* ctx) {
	LMX_CHECK_CTX(ctx);
	return cull_flush(ctx);
}

int lmx_cull_compact(LmxContext* ctx) {
	LMX_CHECK_CTX(ctx);
	return flush_impl(ctx, true);
}

int lmx_cull_stats(LmxContext* ctx, uint32_t* n_entities, uint32_t* n_cells, uint32_t* n_chunks) {
	LMX_CHECK_CTX(ctx);
	if (int rc = flush_impl(ctx, true)) return rc; // the cell count below is that of the sorted layout: fold the overflow in first
	const CullState& cs = ctx->cull;
	if (n_entities) *n_entities = (uint32_t)(cs.recs.size() + cs.dyn.size());
	if (n_cells) *n_cells = cs.n_cells - cs.n_dead_cells;
	if (n_chunks) *n_chunks = (cs.out_total + CHUNK - 1) / CHUNK;
	return LMX_OK;
}

// What the device layout's per-tile tables look like: *cell_key_bytes = 8 (keys relative to the tile's box: every tile spans <= 65535 cell indices per
// axis) or 16; *table_bytes = the cell keys + tile tables + chunk headers a cull of the whole static set reads besides spheres and ids.
int lmx_cull_layout_info(LmxContext* ctx, uint32_t* cell_key_bytes, uint64_t* table_bytes) {
	LMX_CHECK_CTX(ctx);
	if (int rc = flush_impl(ctx, true)) return rc;
	const CullState& cs = ctx->cull;
	const uint32_t kb = cs.keys_packed ? (uint32_t)sizeof(PackedCellKey) : (uint32_t)sizeof(CellKey);
	if (cell_key_bytes) *cell_key_bytes = kb;
	if (table_bytes) { // (the 2048-sphere tiles' tables: what the 1-frustum kernels walk)
		const uint64_t tiles = cs.n_padded / 2048u;
		*table_bytes = tiles * ((uint64_t)cs.tile_cap[1] * kb + 2 * sizeof(uint32_t) + sizeof(TileBox) + sizeof(uint2)) + (uint64_t)(cs.n_padded / CHUNK) * sizeof(ChunkHdr);
	}
	return LMX_OK;
}

int lmx_cull_update_stats(LmxContext* ctx, uint32_t* n_static, uint32_t* n_dynamic_bound, uint32_t* n_overflow, uint32_t* n_tombstones) {
	LMX_CHECK_CTX(ctx);
	const CullState& cs = ctx->cull;
	if (n_static) *n_static = (uint32_t)cs.recs.size();
	if (n_dynamic_bound) *n_dynamic_bound = (uint32_t)(cs.dyn.size() - cs.n_unbound);
	if (n_overflow) *n_overflow = cs.n_unbound;
	if (n_tombstones) *n_tombstones = cs.n_tombstones;
	return LMX_OK;
}

// Fraction of the static set's bounding box that the frustum's own bounding box (its 8 corner points) overlaps: a cheap, stateless
// predictor of how many tiles survive the tile-level test. Only used to pick between kernel variants that return identical results.
static double frustum_box_overlap(const CullState& cs, const LmxShiftedFrustum& f) {
	if (cs.big_tile_fraction > 0.5) return 1.0; // tiles that hold big spheres are never rejected as a whole
	double vol_scene = 1, vol_overlap = 1;
	for (int a = 0; a < 3; ++a) {
		double lo = INFINITY, hi = -INFINITY;
		for (int k = 0; k < 8; ++k) {
			const double p = f.origin[a] + (double)f.points[k][a];
			lo = std::min(lo, p);
			hi = std::max(hi, p);
		}
		const double extent = cs.scene_hi[a] - cs.scene_lo[a];
		if (!(extent > 0) || !(hi >= lo)) return 1.0; // empty set / non-finite corners: no prediction
		vol_scene *= extent;
		vol_overlap *= std::max(0.0, std::min(hi, cs.scene_hi[a]) - std::max(lo, cs.scene_lo[a]));
	}
	return vol_overlap / vol_scene;
}

int lmx_cull(LmxContext* ctx, uint32_t view, const LmxShiftedFrustum* frusta, uint32_t n_frusta, uint8_t type) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_CAPACITY, "view %u >= LMX_MAX_VIEWS", view);
	if (!frusta || n_frusta == 0 || n_frusta > LMX_MAX_FRUSTA) return fail(ctx, LMX_ERR_CAPACITY, "n_frusta %u not in [1,%d]", n_frusta, LMX_MAX_FRUSTA);
	if (type != LMX_TYPE_ALL && type >= MAX_TYPES) return fail(ctx, LMX_ERR_CAPACITY, "type %u >= LMX_MAX_TYPES", type);
	if (int rc = cull_flush(ctx)) return rc;
	CullState& cs = ctx->cull;
	CullView& v = cs.views[view];
	if (v.ext_out && v.ext_out_cap < (size_t)cs.out_total * n_frusta)
		return fail(ctx, LMX_ERR_CAPACITY, "bound output holds %zu ids, need %zu", v.ext_out_cap, (size_t)cs.out_total * n_frusta);
	const uint32_t cnt_frustum_stride = cs.n_shards * cs.cnt_pad;
	const uint32_t cnt_words = std::max(1u, MAX_FRUSTA * cnt_frustum_stride);
	if (v.cnt_words != cnt_words) { // first cull on this view / the shard layout changed: both halves start from zero
		LMX_HIP(ctx, v.counts.reserve(2 * (size_t)cnt_words));
		v.cnt_words = cnt_words;
		v.flip = 0;
		LMX_HIP(ctx, hipMemsetAsync(v.counts.p, 0, 2 * (size_t)cnt_words * sizeof(uint32_t), ctx->stream));
		v.next_half_is_zero = true;
	}
	LMX_HIP(ctx, v.out.reserve(std::max<size_t>((size_t)cs.out_total * n_frusta, 1)));
	if (cs.emit_slots) LMX_HIP(ctx, v.out_slots.reserve(std::max<size_t>((size_t)cs.out_total * n_frusta, 1)));
	v.has_slots = cs.emit_slots;
	v.n_frusta = n_frusta;
	v.out_stride = cs.out_total;
	v.valid = v.finalized = v.consolidated = false;
	for (int t = 0; t < MAX_TYPES; ++t) {
		v.out_start[t] = cs.type_start[t];
		v.out_cap[t] = cs.type_cap[t];
	}
	FrustaArg fr;
	memset(&fr, 0, sizeof(fr));
	for (uint32_t f = 0; f < n_frusta; ++f) fr.f[f] = to_dev_frustum(frusta[f]);

	uint32_t ent_begin = 0, ent_end = cs.n_padded, dyn_begin = 0, dyn_end = cs.dyn_padded;
	if (type != LMX_TYPE_ALL) {
		ent_begin = cs.tt.ent_start[type];
		ent_end = cs.tt.ent_end[type];
		dyn_begin = cs.dyn_tt.ent_start[type];
		dyn_end = cs.dyn_tt.ent_end[type];
	}
	// counters: this cull uses the half the previous one cleared; its first static launch clears the other half
	v.flip ^= 1u;
	if (!v.next_half_is_zero) LMX_HIP(ctx, hipMemsetAsync(v.counts_ptr(), 0, (size_t)cnt_words * sizeof(uint32_t), ctx->stream));
	v.next_half_is_zero = ent_end > ent_begin;
	CullOut out;
	out.ids = v.out.p;
	out.stride = v.out_stride;
	out.win_base = cs.d_win_base.p;
	out.counts = v.counts_ptr();
	out.cnt_pad = cs.cnt_pad;
	out.cnt_frustum_stride = cnt_frustum_stride;
	out.counts_next = v.counts_other();
	out.n_zero = cnt_words;
	out.slots = cs.emit_slots ? v.out_slots.p : nullptr;
	CullDeviceView dv = static_view(cs);
	for (int k = 0; k < 3; ++k) dv.tile_out[k] = cs.d_tile_out[k].p;
	// The kernel is latency-bound for small frusta: wide variants (many frusta per pass) hold more state per wave and run at lower
	// occupancy, so a batch is split into passes of at most `pass_width` frusta.
	// pass_width 0 = automatic: ONE launch for all frusta of the call up to 32 M spheres, frustum by frustum above. Every launch of this
	// latency-bound kernel costs its floor (launch + one round of block start-ups), and since round 4's rework of the several-frusta kernel
	// one pass over the spheres beats eight at 10 M in every regime measured (profiles/r04/width_rule_call39.txt: a frame's 6 views
	// 66 -> 39 us, 8 small cascades 82 -> 49; every sphere tested against 8 frusta 298 -> 141, cull8_pass_widths_call23_*.txt). At 100 M
	// it is the other way round (6 views 185 vs 207 us, config 5's cascades 281 vs 373): the several-frusta kernel walks 1024-sphere tiles
	// with 28 KiB of LDS each - 98 k blocks, five resident per CU - and the blocks that only reject their tile are what the launch is
	// made of there; the 1-frustum kernels walk 2048- / 4096-sphere tiles, eight blocks per CU.
	const uint32_t pass_width = cs.pass_width ? cs.pass_width : (ent_end - ent_begin <= (1u << 25) ? n_frusta : 1u);
	for (uint32_t f0 = 0; f0 < n_frusta; f0 += pass_width) {
		const uint32_t fw = std::min(pass_width, n_frusta - f0);
		FrustaArg sub;
		memset(&sub, 0, sizeof(sub));
		for (uint32_t k = 0; k < fw; ++k) sub.f[k] = fr.f[f0 + k];
		CullOut po = out;
		po.ids = out.ids + (size_t)f0 * out.stride;
		if (out.slots) po.slots = out.slots + (size_t)f0 * out.stride;
		po.counts = out.counts + (size_t)f0 * cnt_frustum_stride;
		if (f0 != 0) { // the first pass of the cull has cleared the next cull's counters already
			po.counts_next = nullptr;
			po.n_zero = 0;
		}
		// 2048-sphere tiles of 4 waves x 8 chunks measured best in every regime (default camera, all-accept, all-test; 10 M and 100 M).
		// With all 8 chunks' loads in flight (variant 4, 66 VGPRs) a launch in which few tiles survive the tile-level test is 7 % shorter
		// (its duration is the latency of the surviving tiles), a launch that streams the whole set 2 % longer: picked by how much of the
		// set's bounding box the frustum's bounding box overlaps.
		const int variant = cs.tile_variant >= 0 ? cs.tile_variant : (fw == 1 && frustum_box_overlap(cs, frusta[f0]) < 0.25 ? 4 : 1);
		ProfScope ps(ctx, LMX_K_CULL_SPHERES, true);
		po.ev_start = ps.slot.a;
		po.ev_stop = ps.slot.b;
		const hipError_t launched = launch_cull_tile(ctx->stream, dv, ent_begin, ent_end, cs.tt, sub, (int)fw, po, variant);
		if (launched != hipSuccess) ps.cancel(); // (the launch fills the scope's events itself: none were recorded)
		LMX_HIP(ctx, launched);
	}
	// dynamic set: its own shards of the same rows / counters
	if (dyn_end > dyn_begin) {
		CullOut po = out;
		po.counts_next = nullptr;
		po.n_zero = 0;
		ProfScope ps(ctx, LMX_K_CULL_DYNAMIC);
		LMX_HIP(ctx, launch_cull_dynamic(ctx->stream, dyn_view(cs), dyn_begin, dyn_end, cs.dyn_tt, fr, (int)n_frusta, po));
	}
	v.valid = true;
	v.culled_type = type;
	if (v.ext_out) return cull_view_consolidate(ctx, v); // a bound output receives the contiguous form right away
	return LMX_OK;
}

int lmx_cull_set_pass_width(LmxContext* ctx, uint32_t frusta_per_pass) {
	LMX_CHECK_CTX(ctx);
	if (frusta_per_pass > LMX_MAX_FRUSTA) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "pass width %u not in [0,%d]", frusta_per_pass, LMX_MAX_FRUSTA);
	ctx->cull.pass_width = frusta_per_pass;
	return LMX_OK;
}

int lmx_cull_set_option(LmxContext* ctx, int option, int value) {
	LMX_CHECK_CTX(ctx);
	CullState& cs = ctx->cull;
	switch (option) {
		case LMX_CULL_OPT_TILE_VARIANT:
			if (value != -1 && value != 1 && value != 4) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "tile variant %d: -1 (auto), 1 (streaming) or 4 (all loads in flight)", value);
			cs.tile_variant = value;
			return LMX_OK;
		case LMX_CULL_OPT_AUTO_COMPACTION: cs.auto_compaction = value != 0; return LMX_OK;
		case LMX_CULL_OPT_COMPACTION_MIN:
			if (value < 1) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "compaction minimum %d < 1", value);
			cs.compaction_min = (uint32_t)value;
			return LMX_OK;
		case LMX_CULL_OPT_DEVICE_OWNS_BOUND: cs.device_owns_bound = value != 0; return LMX_OK;
		case LMX_CULL_OPT_MAP_ZERO_COPY: cs.map_zero_copy = value != 0; cs.map_zero_copy_max = value > 1 ? (uint32_t)value : (1u << 20); return LMX_OK; // (value > 1: the threshold in ids)
		case LMX_CULL_OPT_ASYNC_COMPACTION:
			if (value) return async_enable(ctx);
			async_disable(cs);
			return LMX_OK;
		case LMX_CULL_OPT_OVERFLOW_RESERVE:
			if (value < 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "overflow reserve %d < 0", value);
			cs.overflow_reserve = (uint32_t)value;
			if (value) {
				cs.dyn_layout_dirty = true; // the next flush lays the dynamic set out with the reserve
				// the host mirror of the overflow gets its room now as well: a std::vector that doubles under an add copies tens of MB
				// at 10 M entities (measured: one 8.6 ms frame in a stream of 2 M adds, the entity -> overflow table crossing 10 M ids)
				const size_t ids = std::max(cs.ent_to_dyn.size(), cs.ent_to_rec.size());
				cs.ent_to_dyn.reserve(ids + (size_t)value);
				if (cs.ent_to_dyn.size() < ids) cs.ent_to_dyn.resize(ids, -1);
				cs.dyn.reserve(cs.dyn.size() + (size_t)value);
			}
			return LMX_OK;
		case LMX_CULL_OPT_MAX_SHARDS:
			if (value < 1 || value > (int)LAYOUT_MAX_SHARDS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "max shards %d not in [1,%u]", value, LAYOUT_MAX_SHARDS);
			cs.max_shards = (uint32_t)value;
			if (cs.built) return recompute_out_layout(ctx);
			return LMX_OK;
		case LMX_CULL_OPT_COUNTER_PAD:
			if (value < 1 || value > 64) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "counter pad %d not in [1,64]", value);
			cs.cnt_pad = (uint32_t)value;
			for (CullView& v : cs.views) {
				v.valid = v.finalized = v.consolidated = false;
				v.cnt_words = 0;
			}
			return LMX_OK;
		default: return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown cull option %d", option);
	}
}

} // extern "C"
