// lmx_capi_cull_async.hip — the asynchronous compaction of the culling system's static set (see lmx_capi_cull.hip for the sets).
//
// ---- asynchronous compaction (LMX_CULL_OPT_ASYNC_COMPACTION) ----------------------------------------------------------------------
// The re-sort of the static set is the one O(n) step of the culling system (0.4-0.5 s at 10 M entities). With this option it runs on a
// worker thread, on a SECOND complete copy of the sets (host mirror + device arrays): the shadow set.
//   * Every effective add / remove / set* / bind of the live set is also appended to an operation log (40 bytes, no lock: the log is
//     handed to the worker once per flush).
//   * A job (requested by lmx_cull_flush when the live set's overflow / tombstones pass the usual thresholds): the worker replays the
//     log onto the shadow set's mirror, folds its overflow into its static mirror, builds and uploads a fresh layout on its own
//     stream, then keeps replaying newer log segments - now as O(1) patches on the shadow's device arrays - until a segment is short.
//   * The swap, on the update thread inside a flush: the last few operations are replayed, the two sets trade places (O(1): vectors and
//     device buffers swap storage), the spheres of hierarchy-bound entities - refreshed on the device, not by the host - are copied
//     device to device from the old set, and the output shards are re-derived. The old live set, which has seen every operation, is
//     the next job's shadow.
// What a frame pays: the log appends, and one swap of a few hundred replayed operations per compaction.
// Entrances from the other culling units: async_enable / async_disable, async_poll (the flush), async_reseed, async_wait_idle.
#include "lmx_cull_host.h"

#include <memory>

using namespace lmx;

namespace {

constexpr size_t ASYNC_LOG_LIMIT = 1u << 20;     // operations (40 MB) the log may hold with no job due before a drain job brings the shadow up to date
constexpr size_t ASYNC_SHORT_SEGMENT = 4096; // a log segment this short ends the catch-up: the swap replays what arrived meanwhile

int async_job(LmxContext* ctx, CullAsync& a) {
	CullSet& sh = a.shadow;
	std::vector<CullOp> seg;
	{
		std::lock_guard<std::mutex> g(a.mu);
		seg.swap(a.log_shared);
	}
	// 1. mirror-only replay (no patches: the layout is about to be rebuilt), fold, rebuild both sets of the shadow
	sh.structure_dirty = true;
	sh.dyn_layout_dirty = true;
	clear_static_queues(sh);
	sh.q_dyn.clear();
	if (int rc = async_replay(ctx, sh, seg.data(), seg.size())) return rc;
	if (a.drain_only) return LMX_OK; // the shadow's mirror is current again; no re-sort was due
	fold_overflow(sh);
	if (a.swapped_pending) { // kernels enqueued on the context's stream before the last swap may still read what is now the shadow set
		LMX_HIP(ctx, hipStreamWaitEvent(a.stream, a.swapped, 0));
		a.swapped_pending = false;
	}
	if (int rc = rebuild_static_on(ctx, sh, a.stream, a.overflow_reserve, &a.uploader)) return rc;
	if (int rc = rebuild_dynamic_on(ctx, sh, a.stream, a.overflow_reserve, &a.uploader)) return rc;
	// 2. catch up: newer segments as O(1) patches on the shadow's own device arrays
	for (int round = 0; round < 64; ++round) {
		seg.clear();
		{
			std::lock_guard<std::mutex> g(a.mu);
			seg.swap(a.log_shared);
		}
		if (int rc = async_replay(ctx, sh, seg.data(), seg.size())) return rc;
		if (sh.dyn_layout_dirty) { // a type's region of the shadow's dynamic set ran full during the replay
			if (int rc = rebuild_dynamic_on(ctx, sh, a.stream, a.overflow_reserve, &a.uploader)) return rc;
		}
		if (int rc = apply_patches_on(ctx, sh, a.stream, false)) return rc;
		if (seg.size() < ASYNC_SHORT_SEGMENT) break;
	}
	// 3. entity -> dynamic slot of the shadow set, for the device-to-device copy of bound spheres at the swap
	a.n_new_slot = 0;
	bool any_bound = false;
	for (const DynRec& r : sh.dyn) any_bound = any_bound || r.bound;
	if (any_bound) {
		std::vector<int32_t> slot(sh.ent_to_dyn.size(), -1);
		for (const DynRec& r : sh.dyn)
			if (r.slot != DYN_NO_SLOT) slot[r.entity] = (int32_t)r.slot;
		LMX_HIP(ctx, a.d_new_slot.reserve(std::max<size_t>(slot.size(), 1)));
		if (!slot.empty()) LMX_HIP(ctx, upload_via(&a.uploader, a.d_new_slot.p, slot.data(), slot.size() * sizeof(int32_t), a.stream));
		LMX_HIP(ctx, hipStreamSynchronize(a.stream));
		a.n_new_slot = (uint32_t)slot.size();
	}
	LMX_HIP(ctx, hipStreamSynchronize(a.stream));
	return LMX_OK;
}

void async_worker(LmxContext* ctx, CullAsync* a) {
	(void)hipSetDevice(ctx->device);
	t_layout_thread_cap = 8; // a background re-sort: a quarter of what a synchronous build takes
	t_fail_sink = &a->error; // the worker's errors must not land in LmxContext::error (the update thread may be writing it): fail() honours this
	for (;;) {
		{
			std::unique_lock<std::mutex> g(a->mu);
			a->cv.wait(g, [&] { return a->state == CullAsync::REQUESTED || a->state == CullAsync::QUIT; });
			if (a->state == CullAsync::QUIT) return;
			a->state = CullAsync::RUNNING;
		}
		a->error.clear();
		const int rc = async_job(ctx, *a);
		std::lock_guard<std::mutex> g(a->mu);
		if (a->state == CullAsync::QUIT) return;
		if (rc != LMX_OK) a->state = CullAsync::FAILED;
		else if (a->drain_only) {
			a->state = CullAsync::IDLE;
			a->drains++;
			a->cv_idle.notify_all();
			continue;
		} else a->state = CullAsync::READY;
		a->jobs_done++;
		a->cv_idle.notify_all(); // (async_wait_idle)
	}
}

// update thread: hand the operations of this flush to the log the worker reads
void async_publish_log(CullAsync& a) {
	if (a.log_local.empty()) return;
	std::lock_guard<std::mutex> g(a.mu);
	a.log_shared.insert(a.log_shared.end(), a.log_local.begin(), a.log_local.end());
	a.log_local.clear();
}

CullAsync::State async_state(CullAsync& a) {
	std::lock_guard<std::mutex> g(a.mu);
	return a.state;
}

// update thread, inside a flush, the worker's job is READY: the sets trade places
int async_swap(LmxContext* ctx) {
	CullState& cs = ctx->cull;
	CullAsync& a = *cs.async;
	CullSet& sh = a.shadow;
	// what happened since the worker's last segment (normally a frame or two of operations)
	std::vector<CullOp> tail;
	{
		std::lock_guard<std::mutex> g(a.mu);
		tail.swap(a.log_shared);
	}
	tail.insert(tail.end(), a.log_local.begin(), a.log_local.end());
	a.log_local.clear();
	a.ops_replayed_at_swap += tail.size();
	if (int rc = async_replay(ctx, sh, tail.data(), tail.size())) return rc;
	if (sh.dyn_layout_dirty) {
		if (int rc = rebuild_dynamic_on(ctx, sh, ctx->stream, cs.overflow_reserve)) return rc;
		a.n_new_slot = 0; // slots moved: fall back to the host copy of the bound spheres below
	}
	if (int rc = apply_patches_on(ctx, cs, ctx->stream, true)) return rc;      // the live set's pending patches (its device ids / positions are read below)
	if (int rc = apply_patches_on(ctx, sh, ctx->stream, true)) return rc;      // ordered behind the worker's uploads: its stream was synchronised before READY
	// spheres of hierarchy-bound entities live on the device (k_sphere_refresh): old set -> new set, slot by slot through the entity id
	bool any_bound = false;
	for (const DynRec& r : sh.dyn) {
		if (r.bound) {
			any_bound = true;
			break;
		}
	}
	if (any_bound) {
		if (a.n_new_slot && cs.dyn_padded) {
			LMX_HIP(ctx, launch_dyn_carry_over(ctx->stream, dyn_view(cs), dyn_view(sh), a.d_new_slot.p, a.n_new_slot));
		} else {
			if (int rc = cull_dyn_sync_mirror(ctx)) return rc; // (rare path: O(bound entities) on the host)
			for (DynRec& r : sh.dyn) {
				uint32_t idx;
				if (!r.bound || locate(cs, r.entity, &idx) != Where::DYNAMIC) continue;
				const DynRec& o = cs.dyn[idx];
				r.pos[0] = o.pos[0]; r.pos[1] = o.pos[1]; r.pos[2] = o.pos[2];
				r.radius = o.radius;
				queue_dyn_patch(sh, r, true);
			}
			if (int rc = apply_patches_on(ctx, sh, ctx->stream, true)) return rc;
		}
	}
	if (int rc = keys_before_layout_change(ctx)) return rc; // (reads the OLD set's slot -> id array)
	const uint64_t generation = std::max(cs.dyn_generation, sh.dyn_generation) + 1;
	static_assert(std::is_nothrow_move_constructible<CullSet>::value && std::is_nothrow_move_assignable<CullSet>::value, "the sets trade places by moving their storage, never by copying it");
	std::swap(static_cast<CullSet&>(cs), sh); // O(1): vectors and device buffers move their storage
	cs.layout_generation = g_layout_generation++;
	cs.dyn_generation = generation; // the world's binding tables (slots of bound entities) are re-derived at the next propagation
	sh.dyn_generation = generation;
	if (any_bound) cs.dyn_mirror_stale = true; // the host copies of bound spheres are older than the device's
	// the old live set is the next shadow: it has seen every operation; its device arrays are dead weight until the next job rebuilds them
	sh.structure_dirty = true;
	sh.dyn_layout_dirty = true;
	clear_static_queues(sh);
	sh.q_dyn.clear();
	sh.q_sphere_at.clear();
	if (!a.swapped) LMX_HIP(ctx, hipEventCreateWithFlags(&a.swapped, hipEventDisableTiming));
	LMX_HIP(ctx, hipEventRecord(a.swapped, ctx->stream));
	a.swapped_pending = true;
	a.swaps++;
	{
		std::lock_guard<std::mutex> g(a.mu);
		a.state = CullAsync::IDLE;
	}
	return recompute_out_layout(ctx);
}

} // namespace

namespace lmx {

// The shadow set := a copy of the live set's host mirror (O(n), once: when the option is switched on, after lmx_cull_build and after
// a synchronous compaction); its device arrays are rebuilt by the first job anyway.
void async_reseed(CullState& cs) {
	CullAsync& a = *cs.async;
	CullSet& sh = a.shadow;
	sh.recs = cs.recs;
	sh.ent_to_rec = cs.ent_to_rec;
	sh.rec_slot.clear();
	sh.dyn = cs.dyn;
	sh.ent_to_dyn = cs.ent_to_dyn;
	sh.n_unbound = cs.n_unbound;
	sh.built = cs.built;
	sh.structure_dirty = true;
	sh.dyn_layout_dirty = true;
	sh.n_tombstones = 0;
	clear_static_queues(sh);
	sh.q_dyn.clear();
	a.log_local.clear();
	std::lock_guard<std::mutex> g(a.mu);
	a.log_shared.clear();
	if (a.state != CullAsync::QUIT) a.state = CullAsync::IDLE; // (no job runs here: every caller has seen the last one end)
}

void async_wait_idle(CullAsync& a) { // update thread: let a running job finish (its result is discarded by the caller)
	// (a sleep on the worker's own condition variable, not a yield spin: the caller holds the context's lock for as long as the job
	// runs - 0.5 s at 10 M entities - and should not burn a core next to the worker meanwhile)
	std::unique_lock<std::mutex> g(a.mu);
	a.cv_idle.wait(g, [&] { return a.state != CullAsync::REQUESTED && a.state != CullAsync::RUNNING; });
}

// update thread, every flush of a live layout while the option is on. Returns LMX_OK; *handled = the sets were swapped.
int async_poll(LmxContext* ctx, bool* swapped) {
	CullState& cs = ctx->cull;
	CullAsync& a = *cs.async;
	*swapped = false;
	async_publish_log(a);
	const CullAsync::State st = async_state(a);
	if (st == CullAsync::READY) {
		if (int rc = async_swap(ctx)) { // could not adopt the shadow set: start over from a copy of the live one
			async_reseed(cs);
			return rc;
		}
		*swapped = true;
		return LMX_OK;
	}
	if (st == CullAsync::FAILED) {
		fail(ctx, LMX_ERR_HIP, "asynchronous compaction failed: %s", a.error.c_str());
		async_reseed(cs);
		return LMX_OK; // the live set is intact; the next request starts from a fresh copy
	}
	if (st == CullAsync::IDLE) {
		const bool resort = cs.auto_compaction && wants_compaction(cs);
		// in-cell moves patch the sorted set in place and never make a re-sort due: the log must not grow without bound meanwhile
		size_t backlog;
		{
			std::lock_guard<std::mutex> g(a.mu);
			backlog = a.log_shared.size();
		}
		const bool drain = !resort && backlog > std::max<size_t>(ASYNC_LOG_LIMIT, cs.recs.size() / 4);
		if (resort || drain) {
			a.overflow_reserve = cs.overflow_reserve;
			a.drain_only = drain;
			std::lock_guard<std::mutex> g(a.mu);
			a.state = CullAsync::REQUESTED;
			a.cv.notify_one();
		}
	}
	return LMX_OK;
}

int async_enable(LmxContext* ctx) {
	CullState& cs = ctx->cull;
	if (cs.async) return LMX_OK;
	auto a = std::make_unique<CullAsync>(); // (a failure below frees what exists so far: ~CullAsync, ~PinnedUploader)
	hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
	if (e != hipSuccess) return fail(ctx, LMX_ERR_HIP, "hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
	e = a->uploader.init(a->stream);
	if (e != hipSuccess) return fail(ctx, LMX_ERR_HIP, "pinned staging for the asynchronous compaction: %s", hipGetErrorString(e));
	cs.async = a.release();
	async_reseed(cs);
	cs.async->worker = std::thread(async_worker, ctx, cs.async);
	return LMX_OK;
}

void async_disable(CullState& cs) {
	CullAsync* a = cs.async;
	if (!a) return;
	async_wait_idle(*a);
	cs.async = nullptr;
	delete a;
}

CullAsync::~CullAsync() {
	{
		std::lock_guard<std::mutex> g(mu);
		state = QUIT;
		cv.notify_one();
	}
	if (worker.joinable()) worker.join();
	if (stream) (void)hipStreamDestroy(stream);
	if (swapped) (void)hipEventDestroy(swapped);
}

void cull_async_shutdown(LmxContext* ctx) { async_disable(ctx->cull); }

} // namespace lmx

extern "C" {

int lmx_cull_async_stats(LmxContext* ctx, int* state, uint64_t* jobs, uint64_t* swaps, uint64_t* ops_replayed_at_swaps, uint64_t* log_drains) {
	if (!ctx) return LMX_ERR_INVALID_ARGUMENT;
	CullAsync* a = ctx->cull.async;
	if (state) *state = a ? (int)async_state(*a) : -1;
	if (a) {
		std::lock_guard<std::mutex> g(a->mu);
		if (jobs) *jobs = a->jobs_done;
		if (log_drains) *log_drains = a->drains;
	} else {
		if (jobs) *jobs = 0;
		if (log_drains) *log_drains = 0;
	}
	if (swaps) *swaps = a ? a->swaps : 0;
	if (ops_replayed_at_swaps) *ops_replayed_at_swaps = a ? a->ops_replayed_at_swap : 0;
	return LMX_OK;
}

} // extern "C"
