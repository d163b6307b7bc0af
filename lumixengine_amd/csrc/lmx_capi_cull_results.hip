// lmx_capi_cull_results.hip — the result side of the culling system (see lmx_capi_cull.hip): per-type totals and contiguous lists of a
// view's shard windows, the host reads, the map_begin / map_end ticket protocol, the packed device record, view slots, bound outputs.
// Everything here only reads CullState's output layout and a CullView.
#include "lmx_context.h"

#include <chrono>

using namespace lmx;

namespace lmx {

int cull_view_finalize(LmxContext* ctx, CullView& v) {
	CullState& cs = ctx->cull;
	if (v.finalized) return LMX_OK;
	LMX_HIP(ctx, v.totals.reserve(MAX_FRUSTA * MAX_TYPES));
	LMX_HIP(ctx, v.pref.reserve(std::max<size_t>((size_t)MAX_FRUSTA * cs.n_shards, 1)));
	uint32_t* totals = v.ext_counts ? v.ext_counts : v.totals.p;
	LMX_HIP(ctx, launch_cull_finalize(ctx->stream, v.counts_ptr(), cs.cnt_pad, cs.n_shards * cs.cnt_pad, cs.d_shard_type.p, cs.n_shards, v.n_frusta, totals, v.pref.p, nullptr));
	v.finalized = true;
	return LMX_OK;
}

int cull_view_consolidate(LmxContext* ctx, CullView& v) {
	CullState& cs = ctx->cull;
	if (v.consolidated) return LMX_OK;
	if (int rc = cull_view_finalize(ctx, v)) return rc;
	int32_t* dst = v.ext_out;
	if (!dst) {
		LMX_HIP(ctx, v.cons.reserve(std::max<size_t>((size_t)v.out_stride * v.n_frusta, 1)));
		dst = v.cons.p;
	}
	if (v.has_slots) LMX_HIP(ctx, v.cons_slots.reserve(std::max<size_t>((size_t)v.out_stride * v.n_frusta, 1))); // the same gather for the slots, in the same launch
	LMX_HIP(ctx, launch_cull_consolidate(ctx->stream, v.out.p, v.out_stride, cs.d_win_base.p, v.counts_ptr(), cs.cnt_pad, cs.n_shards * cs.cnt_pad, cs.d_shard_type.p,
		cs.d_type_start.p, 0, v.pref.p, cs.n_shards, v.n_frusta, cs.max_shard_cap, dst, v.out_stride, 0xffffffffu, v.has_slots ? v.out_slots.p : nullptr,
		v.has_slots ? v.cons_slots.p : nullptr));
	v.consolidated = true;
	return LMX_OK;
}

} // namespace lmx

extern "C" {

int lmx_cull_counts(LmxContext* ctx, uint32_t view, uint32_t* counts) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS || !counts) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view/counts");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (int rc = cull_view_finalize(ctx, v)) return rc;
	uint32_t all[MAX_FRUSTA * MAX_TYPES];
	LMX_HIP(ctx, read_back(all, v.totals_ptr(), (size_t)v.n_frusta * MAX_TYPES, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	memcpy(counts, all, sizeof(uint32_t) * v.n_frusta * MAX_TYPES);
	return LMX_OK;
}

int lmx_cull_read(LmxContext* ctx, uint32_t view, uint32_t frustum, uint8_t type, int32_t* out_ids, uint32_t cap, uint32_t* out_count) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta || type >= MAX_TYPES) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u / type %u out of range", frustum, type);
	if (int rc = cull_view_consolidate(ctx, v)) return rc;
	uint32_t c = 0;
	LMX_HIP(ctx, read_back(&c, v.totals_ptr() + frustum * MAX_TYPES + type, 1, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (out_count) *out_count = c;
	if (c > v.out_cap[type]) return fail(ctx, LMX_ERR_HIP, "corrupt count %u > %u", c, v.out_cap[type]);
	if (!out_ids || c == 0) return LMX_OK;
	if (c > cap) return fail(ctx, LMX_ERR_CAPACITY, "need room for %u ids, got %u", c, cap);
	LMX_HIP(ctx, read_back(out_ids, v.cons_ptr() + (size_t)frustum * v.out_stride + v.out_start[type], c, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return LMX_OK;
}

// All types of one frustum with two host waits (totals, then every non-empty type's ids): what the CullResult adapter needs.
int lmx_cull_read_all(LmxContext* ctx, uint32_t view, uint32_t frustum, int32_t* out_ids, uint32_t cap, uint32_t* out_counts) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS || !out_counts) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view / counts");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u out of range", frustum);
	if (int rc = cull_view_consolidate(ctx, v)) return rc;
	LMX_HIP(ctx, read_back(out_counts, v.totals_ptr() + frustum * MAX_TYPES, MAX_TYPES, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	size_t total = 0;
	for (int t = 0; t < MAX_TYPES; ++t) {
		if (out_counts[t] > v.out_cap[t]) return fail(ctx, LMX_ERR_HIP, "corrupt count %u > %u", out_counts[t], v.out_cap[t]);
		total += out_counts[t];
	}
	if (!total) return LMX_OK;
	if (!out_ids || total > cap) return fail(ctx, LMX_ERR_CAPACITY, "need room for %zu ids, got %u", total, cap);
	size_t at = 0;
	for (int t = 0; t < MAX_TYPES; ++t) {
		if (!out_counts[t]) continue;
		LMX_HIP(ctx, read_back(out_ids + at, v.cons_ptr() + (size_t)frustum * v.out_stride + v.out_start[t], out_counts[t], ctx->stream));
		at += out_counts[t];
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return LMX_OK;
}

// All types of one frustum with (normally) ONE host wait: the gather kernels pack [counts | ids, type 0 first] into one device
// record, and the copy into pinned host memory is enqueued right behind them for as many ids as the previous call on this view
// returned (+25 %): frames are coherent, so the guess almost always covers the list; when it does not, the rest follows with a second
// wait. The caller reads the ids in place: *out_ids stays valid until the next lmx_cull_map_all on this view.
// (Letting the gather kernel store straight into mapped host memory was measured too: 4-byte stores over PCIe, 0.49 ms for 334 k ids.)
// Records [MAX_TYPES counts | ids, types back to back] of frusta [first, first + n) of a view, each packed by one k_cull_pack launch into
// its own area of map_rec and copied into pinned host memory - counts + the first map_guess ids before the count is known - with ONE
// host wait for all of them (a second one only for a frustum whose list outgrew its guess, this frame only).
// The host read of a view's result in two halves, so that render jobs culling different views only serialise on the ENQUEUE:
//   cull_map_begin  (context lock held) packs the shard windows into one record per frustum, enqueues its copy into the view's pinned
//                   buffer - as many ids as the last frame on that view needed + 25 % - and records the view's event behind it;
//   cull_map_end    (no lock needed: touches this view's buffers only) waits for THAT event, reads the counts, and - only if the list
//                   outgrew the guess - takes the lock for a second copy.
static int cull_map_begin(LmxContext* ctx, CullView& v, uint32_t first, uint32_t n) {
	CullState& cs = ctx->cull;
	const size_t need = (size_t)MAX_TYPES + v.out_stride; // words per record area
	if (v.map_words < need || v.map_frusta < v.n_frusta) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // nothing may still write the old buffer
		if (v.map_host) LMX_HIP(ctx, hipHostFree(v.map_host));
		v.map_host = nullptr;
		v.map_words = 0;
		const size_t want = need + need / 4 + 1024;
		const size_t areas = std::max<size_t>(v.n_frusta, v.map_frusta);
		LMX_HIP(ctx, hipHostMalloc(&v.map_host, want * areas * sizeof(int32_t), hipHostMallocDefault));
		LMX_HIP(ctx, v.map_rec.reserve(want * areas));
		v.map_words = want;
		v.map_frusta = areas;
	}
	if (!v.map_event) LMX_HIP(ctx, hipEventCreateWithFlags(&v.map_event, hipEventDisableTiming));
	const uint32_t cnt_frustum_stride = cs.n_shards * cs.cnt_pad;
	// Lists of up to 1 M ids last frame: k_cull_pack writes the record STRAIGHT into the pinned host buffer (the buffer's device mapping:
	// posted writes over PCIe) - no copy command behind the kernel, whose fixed cost (~10 us of a ~45 us cull of the harness's 40 k-entity
	// scene) is what a host read of a small list consists of; at the headline camera's 334 k ids (1.3 MB) the host read is still 20 us
	// shorter this way (104 against 124 us per cull + read through the Python wrapper, profiles/r04/readback_zero_copy_call43.txt; round 4's
	// first cut stopped at 64 k ids). Larger lists keep the device record + one DMA copy of the ids the last frame needed: a kernel that
	// streams many megabytes over PCIe holds its CUs for the duration.
	int32_t* host_dev = nullptr;
	// (only once a count has been read back on this view: the initial guess says nothing about the list, and a zero-copy record streams
	// ALL its ids over PCIe with the CUs held - a first map of a 10 M-id list would be tens of megabytes of posted writes)
	bool zero_copy = cs.map_zero_copy && v.map_seen;
	for (uint32_t k = 0; k < n && zero_copy; ++k) zero_copy = v.map_guess[first + k].load(std::memory_order_relaxed) <= cs.map_zero_copy_max;
	if (zero_copy && hipHostGetDevicePointer(reinterpret_cast<void**>(&host_dev), v.map_host, 0) != hipSuccess) zero_copy = false;
	CullView::MapTicket& tk = v.ticket;
	tk.n = 0;
	tk.zero_copy = zero_copy;
	tk.host = reinterpret_cast<int32_t*>(v.map_host);
	tk.rec = v.map_rec.p;
	tk.words = v.map_words;
	memcpy(tk.out_cap, v.out_cap, sizeof(tk.out_cap));
	{ // the records of all n frusta: ONE launch (a frame's six views cost six launch gaps otherwise)
		int32_t* rec = (zero_copy ? host_dev : v.map_rec.p) + (size_t)first * v.map_words;
		if (v.map_words > 0xffffffffull) return fail(ctx, LMX_ERR_CAPACITY, "record stride exceeds 32 bits");
		LMX_HIP(ctx, launch_cull_pack(ctx->stream, v.out.p + (size_t)first * v.out_stride, cs.d_win_base.p, v.counts_ptr() + (size_t)first * cnt_frustum_stride, cs.cnt_pad,
			cs.d_shard_type.p, cs.n_shards, cs.max_shard_cap, reinterpret_cast<uint32_t*>(rec), rec + MAX_TYPES, v.out_stride, n, (uint32_t)v.out_stride, cnt_frustum_stride,
			(uint32_t)v.map_words));
	}
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t f = first + k;
		const int32_t* rec = v.map_rec.p + (size_t)f * v.map_words;
		tk.guess[k] = zero_copy ? (size_t)v.out_stride : std::min<size_t>(v.out_stride, v.map_guess[f].load(std::memory_order_relaxed));
		if (!zero_copy)
			LMX_HIP(ctx, hipMemcpyAsync(tk.host + (size_t)f * v.map_words, rec, (MAX_TYPES + tk.guess[k]) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	}
	LMX_HIP(ctx, hipEventRecord(v.map_event, ctx->stream));
	tk.first = first;
	tk.n = n;
	v.map_seen = true; // (the matching map_end reads the counts before the next map_begin on this view can run)
	return LMX_OK;
}

static int cull_map_end(LmxContext* ctx, CullView& v, uint32_t first, uint32_t n, const int32_t** out_ids, uint32_t* out_counts) {
	struct Locked { // (error strings and stream operations belong to the context: taken only on the rare paths)
		LmxContext* c;
		explicit Locked(LmxContext* c_) : c(c_) { c->lock.lock(); }
		~Locked() { c->lock.unlock(); }
	};
	// everything read here is the view's ticket (filled by map_begin under the lock, untouched until the next map_begin on this view), its
	// event and the pinned buffer the ticket names
	const CullView::MapTicket& tk = v.ticket;
	if (!v.map_event || tk.n != n || tk.first != first) {
		Locked l(ctx);
		return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_cull_map_end without a matching lmx_cull_map_begin on this view");
	}
	if (hipEventSynchronize(v.map_event) != hipSuccess) {
		Locked l(ctx);
		return fail(ctx, LMX_ERR_HIP, "waiting for the view's record failed");
	}
	bool more = false;
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t f = first + k;
		int32_t* host = tk.host + (size_t)f * tk.words;
		const uint32_t* h = reinterpret_cast<const uint32_t*>(host);
		size_t total = 0;
		for (int t = 0; t < MAX_TYPES; ++t) {
			if (h[t] > tk.out_cap[t]) {
				Locked l(ctx);
				return fail(ctx, LMX_ERR_HIP, "corrupt count %u > %u", h[t], tk.out_cap[t]);
			}
			out_counts[k * MAX_TYPES + t] = h[t];
			total += h[t];
		}
		if (total > tk.guess[k] && !tk.zero_copy) { // the list outgrew the guess: fetch the rest (second wait, this frame only)
			Locked l(ctx);
			LMX_HIP(ctx, hipSetDevice(ctx->device)); // (this thread may never have selected the context's device)
			LMX_HIP(ctx, hipMemcpyAsync(host + MAX_TYPES + tk.guess[k], tk.rec + (size_t)f * tk.words + MAX_TYPES + tk.guess[k],
				(total - tk.guess[k]) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
			more = true;
		}
		v.map_guess[f].store((uint32_t)std::min<size_t>(total + total / 4 + 1024, 0xffffffffu), std::memory_order_relaxed);
		out_ids[k] = host + MAX_TYPES;
	}
	if (more) {
		Locked l(ctx);
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	v.ticket.n = 0;
	return LMX_OK;
}

static int cull_map_range(LmxContext* ctx, CullView& v, uint32_t first, uint32_t n, const int32_t** out_ids, uint32_t* out_counts) {
	if (int rc = cull_map_begin(ctx, v, first, n)) return rc;
	return cull_map_end(ctx, v, first, n, out_ids, out_counts);
}

// The packed record of one frustum left in HBM, no host wait: what a device-side consumer of "one cull incl. compaction" reads
// (bench.py's timed step; the exchange packs into its own send buffer the same way).
int lmx_cull_pack_device(LmxContext* ctx, uint32_t view, uint32_t frustum, const int32_t** d_record, uint32_t* record_words) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS || !d_record) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view / null output");
	CullState& cs = ctx->cull;
	CullView& v = cs.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u out of range", frustum);
	const size_t need = (size_t)MAX_TYPES + v.out_stride;
	if (v.pack_words < need) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		LMX_HIP(ctx, v.pack_rec.reserve(need + need / 4 + 1024));
		v.pack_words = need + need / 4 + 1024;
	}
	const uint32_t* counts = v.counts_ptr() + (size_t)frustum * cs.n_shards * cs.cnt_pad;
	LMX_HIP(ctx, launch_cull_pack(ctx->stream, v.out.p + (size_t)frustum * v.out_stride, cs.d_win_base.p, counts, cs.cnt_pad, cs.d_shard_type.p, cs.n_shards, cs.max_shard_cap,
		reinterpret_cast<uint32_t*>(v.pack_rec.p), v.pack_rec.p + MAX_TYPES, v.out_stride));
	*d_record = v.pack_rec.p;
	if (record_words) *record_words = (uint32_t)need;
	return LMX_OK;
}

int lmx_cull_map_all(LmxContext* ctx, uint32_t view, uint32_t frustum, const int32_t** out_ids, uint32_t* out_counts) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS || !out_counts || !out_ids) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view / null output");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u out of range", frustum);
	return cull_map_range(ctx, v, frustum, 1, out_ids, out_counts);
}

int lmx_cull_map_many(LmxContext* ctx, uint32_t view, uint32_t n_frusta, const int32_t** out_ids, uint32_t* out_counts) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS || !out_counts || !out_ids) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view / null output");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (n_frusta != v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the view holds %u frusta, not %u", v.n_frusta, n_frusta);
	return cull_map_range(ctx, v, 0, n_frusta, out_ids, out_counts);
}

int lmx_cull_map_begin(LmxContext* ctx, uint32_t view, uint32_t n_frusta) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (n_frusta != v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the view holds %u frusta, not %u", v.n_frusta, n_frusta);
	return cull_map_begin(ctx, v, 0, n_frusta);
}

int lmx_cull_map_end(LmxContext* ctx, uint32_t view, uint32_t n_frusta, const int32_t** out_ids, uint32_t* out_counts) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT; // (LMX_CHECK_CTX selects the context's device: not needed to wait for an event and read host memory)
	if (view >= LMX_MAX_VIEWS || !out_counts || !out_ids) return LMX_ERR_INVALID_ARGUMENT;
	return cull_map_end(ctx, ctx->cull.views[view], 0, n_frusta, out_ids, out_counts);
}

// Result slots that cannot alias (CullingSystem::cull returns an independent list per call, culling_system.cpp:321-369; callers
// pipeline.cpp:1036-1045, :3380, editor/scene_view.cpp:144): a slot handed out here is not handed out again before its holder has
// released it, i.e. before it has copied the ids out of the slot's pinned record. With every slot taken the caller waits for the
// next release - bounded: a holder that never releases turns into LMX_ERR_BUSY, not into a hang.
int lmx_cull_view_acquire(LmxContext* ctx, uint32_t* view, uint32_t timeout_ms) {
	if (!ctx || !view) return LMX_ERR_INVALID_ARGUMENT;
	CullState& cs = ctx->cull;
	std::unique_lock<std::mutex> l(cs.views_mutex);
	constexpr uint32_t ALL = (1u << LMX_MAX_VIEWS) - 1u;
	if ((cs.views_busy & ALL) == ALL) {
		const bool got = cs.views_cv.wait_for(l, std::chrono::milliseconds(timeout_ms), [&] { return (cs.views_busy & ALL) != ALL; });
		if (!got) return LMX_ERR_BUSY; // (no fail(): the error string belongs to the context's lock, which this path never takes)
	}
	for (uint32_t k = 0; k < (uint32_t)LMX_MAX_VIEWS; ++k) { // round robin: consecutive culls of a frame land on different slots (their buffers stay sized for their view)
		const uint32_t s = (cs.views_next + k) % (uint32_t)LMX_MAX_VIEWS;
		if (!((cs.views_busy >> s) & 1u)) {
			cs.views_busy |= 1u << s;
			cs.views_next = (s + 1u) % (uint32_t)LMX_MAX_VIEWS;
			*view = s;
			return LMX_OK;
		}
	}
	return LMX_ERR_BUSY; // (unreachable)
}

int lmx_cull_view_release(LmxContext* ctx, uint32_t view) {
	if (!ctx || view >= (uint32_t)LMX_MAX_VIEWS) return LMX_ERR_INVALID_ARGUMENT;
	CullState& cs = ctx->cull;
	{
		std::lock_guard<std::mutex> l(cs.views_mutex);
		if (!((cs.views_busy >> view) & 1u)) return LMX_ERR_INVALID_ARGUMENT; // released twice / never acquired
		cs.views_busy &= ~(1u << view);
	}
	cs.views_cv.notify_one();
	return LMX_OK;
}

int lmx_cull_bind_output(LmxContext* ctx, uint32_t view, void* d_ids, size_t ids_capacity, void* d_counts) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view");
	if ((d_ids == nullptr) != (d_counts == nullptr)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bind both buffers or neither");
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	CullView& v = ctx->cull.views[view];
	v.ext_out = (int32_t*)d_ids;
	v.ext_out_cap = d_ids ? ids_capacity : 0;
	v.ext_counts = (uint32_t*)d_counts;
	v.valid = v.finalized = v.consolidated = false;
	return LMX_OK;
}

int lmx_cull_device_result(LmxContext* ctx, uint32_t view, uint32_t frustum, const int32_t** d_ids, const uint32_t** d_counts,
	uint32_t* type_offsets, uint32_t* capacity) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view");
	CullView& v = ctx->cull.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u out of range", frustum);
	if (int rc = cull_view_consolidate(ctx, v)) return rc;
	if (d_ids) *d_ids = v.cons_ptr() + (size_t)frustum * v.out_stride;
	if (d_counts) *d_counts = v.totals_ptr();
	if (type_offsets) memcpy(type_offsets, v.out_start, sizeof(v.out_start));
	if (capacity) *capacity = v.out_stride;
	return LMX_OK;
}

int lmx_cull_device_shards(LmxContext* ctx, uint32_t view, uint32_t frustum, LmxCullShards* out) {
	LMX_CHECK_CTX(ctx);
	if (view >= LMX_MAX_VIEWS || !out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad view / out");
	CullState& cs = ctx->cull;
	CullView& v = cs.views[view];
	if (!v.valid) return fail(ctx, LMX_ERR_NOT_BUILT, "view %u holds no cull result", view);
	if (frustum >= v.n_frusta) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frustum %u out of range", frustum);
	out->d_ids = v.out.p + (size_t)frustum * v.out_stride;
	out->d_counts = v.counts_ptr() + (size_t)frustum * cs.n_shards * cs.cnt_pad;
	out->count_stride = cs.cnt_pad;
	out->d_window_start = cs.d_win_base.p;
	out->d_shard_type = cs.d_shard_type.p;
	out->n_shards = cs.n_shards;
	return LMX_OK;
}

} // extern "C"
