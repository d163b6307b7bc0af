// lmx_cull_host.h — what the culling translation units share and nothing else does (internal; lmx_context.h holds what the OTHER
// subsystems call: cull_flush, cull_dyn_sync_mirror, cull_make_dynamic, cull_unbind, cull_view_*, cull_async_shutdown):
//   lmx_capi_cull_set.hip      the host mirror of the two resident sets, its O(1) mutations and the entry points that use only it
//   lmx_capi_cull_async.hip    the asynchronous compaction: shadow set, operation log, worker thread, swap
//   lmx_capi_cull.hip          device upkeep (patches, rebuilds, output layout, flush) and the launch
//   lmx_capi_cull_results.hip  the result side: totals, contiguous lists, host reads, the map protocol, view slots
#pragma once

#include "lmx_context.h"

#include <atomic>
#include <condition_variable>
#include <thread>

namespace lmx {

enum class Where { NONE, STATIC, DYNAMIC };

// ---- asynchronous compaction: types (the machinery is in lmx_capi_cull_async.hip) -----------------------------------------------
enum : uint8_t { OP_ADD, OP_REMOVE, OP_SET, OP_SET_POS, OP_SET_RADIUS, OP_BIND, OP_UNBIND };
struct CullOp { // one EFFECTIVE mutation of the live set, replayed onto the shadow set
	double pos[3];
	float radius;
	int32_t entity;
	uint8_t op, type;
};

// Host -> device copies of the asynchronous compaction's worker go through two pinned staging buffers, chunk by chunk: a
// hipMemcpyAsync from PAGEABLE memory is staged by the runtime in a way that held up the context's own stream for the length of the
// whole upload (measured: one 32 ms frame while 400 MB of a re-sorted 12 M-entity set went up; tools/scratch/async_stream_probe.py).
struct PinnedUploader {
	static constexpr size_t CHUNK = 4u << 20;
	void* buf[2] = {nullptr, nullptr};
	hipEvent_t ev[2] = {nullptr, nullptr};
	bool used[2] = {false, false};
	int k = 0;
	hipStream_t stream = nullptr;
	PinnedUploader() = default;
	PinnedUploader(const PinnedUploader&) = delete;
	PinnedUploader& operator=(const PinnedUploader&) = delete;
	~PinnedUploader() {
		for (int i = 0; i < 2; ++i) {
			if (buf[i]) (void)hipHostFree(buf[i]);
			if (ev[i]) (void)hipEventDestroy(ev[i]);
		}
	}
	hipError_t init(hipStream_t s) { // (allocations that may fail: not a constructor's job in a library without exceptions; a half-done init is freed by the destructor)
		stream = s;
		for (int i = 0; i < 2; ++i) {
			hipError_t e = hipHostMalloc(&buf[i], CHUNK, hipHostMallocDefault);
			if (e != hipSuccess) return e;
			e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
			if (e != hipSuccess) return e;
		}
		return hipSuccess;
	}
	hipError_t copy(void* dst, const void* src, size_t bytes) {
		for (size_t off = 0; off < bytes; off += CHUNK) {
			const size_t n = std::min(CHUNK, bytes - off);
			if (used[k]) {
				hipError_t e = hipEventSynchronize(ev[k]);
				if (e != hipSuccess) return e;
			}
			memcpy(buf[k], (const char*)src + off, n);
			hipError_t e = hipMemcpyAsync((char*)dst + off, buf[k], n, hipMemcpyHostToDevice, stream);
			if (e != hipSuccess) return e;
			e = hipEventRecord(ev[k], stream);
			if (e != hipSuccess) return e;
			used[k] = true;
			k ^= 1;
		}
		return hipSuccess;
	}
};
inline hipError_t upload_via(PinnedUploader* up, void* dst, const void* src, size_t bytes, hipStream_t stream) {
	return up ? up->copy(dst, src, bytes) : hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
}

struct CullAsync {
	enum State : int { IDLE, REQUESTED, RUNNING, READY, FAILED, QUIT };
	CullSet shadow;                 // owned by the worker while RUNNING, by the update thread otherwise
	std::vector<CullOp> log_local;  // update thread only: operations since the last hand-over
	std::vector<CullOp> log_shared; // under `mu`: operations the shadow set has not seen yet
	std::mutex mu;
	std::condition_variable cv;
	std::condition_variable cv_idle; // signalled by the worker when a job ends (async_wait_idle sleeps on it)
	State state = IDLE;             // under `mu`
	std::thread worker;
	hipStream_t stream = nullptr;   // the worker's own (non-blocking) stream
	PinnedUploader uploader;        // its host -> device copies go through pinned staging buffers
	hipEvent_t swapped = nullptr;   // recorded on the context's stream when the sets trade places: the worker's uploads into what WAS the live set wait for it
	bool swapped_pending = false;
	uint32_t overflow_reserve = 0;  // copy of the tuning value for the job in flight
	bool drain_only = false;        // the job in flight only brings the shadow's mirror up to date (the log had grown long with no re-sort due)
	uint64_t drains = 0;
	std::string error;              // the worker's failure (state FAILED)
	DevBuf<int32_t> d_new_slot;     // entity -> dynamic slot of the shadow set (bound spheres are copied device to device at the swap)
	uint32_t n_new_slot = 0;
	uint64_t jobs_done = 0, swaps = 0, ops_replayed_at_swap = 0;
	CullAsync() = default;
	~CullAsync(); // lmx_capi_cull_async.hip: stops and joins the worker, destroys the stream and the event
};

inline void async_log(CullState& cs, uint8_t op, int32_t entity, uint8_t type, const double* pos, float radius) {
	if (!cs.async) return;
	CullOp o;
	o.pos[0] = pos ? pos[0] : 0.0;
	o.pos[1] = pos ? pos[1] : 0.0;
	o.pos[2] = pos ? pos[2] : 0.0;
	o.radius = radius;
	o.entity = entity;
	o.op = op;
	o.type = type;
	cs.async->log_local.push_back(o);
}

inline Where locate(const CullSet& cs, int32_t entity, uint32_t* index) {
	if (entity < 0) return Where::NONE;
	if ((size_t)entity < cs.ent_to_rec.size() && cs.ent_to_rec[entity] >= 0) {
		*index = (uint32_t)cs.ent_to_rec[entity];
		return Where::STATIC;
	}
	if ((size_t)entity < cs.ent_to_dyn.size() && cs.ent_to_dyn[entity] >= 0) {
		*index = (uint32_t)cs.ent_to_dyn[entity];
		return Where::DYNAMIC;
	}
	return Where::NONE;
}

inline bool layout_live(const CullSet& cs) { return cs.built && !cs.structure_dirty; }

inline void clear_static_queues(CullSet& cs) {
	for (const PatchSphere& p : cs.q_sphere) if (p.slot < cs.q_sphere_at.size()) cs.q_sphere_at[p.slot] = ~0u;
	cs.q_sphere.clear();
	cs.q_id.clear();
}
inline void clear_dyn_queue(CullSet& cs) {
	for (const PatchDyn& p : cs.q_dyn) cs.q_dyn_at[p.slot] = ~0u;
	cs.q_dyn.clear();
}

inline DynDeviceView dyn_view(const CullSet& cs) {
	DynDeviceView dd;
	dd.px = cs.dyn_px.p;
	dd.py = cs.dyn_py.p;
	dd.pz = cs.dyn_pz.p;
	dd.radius = cs.dyn_radius.p;
	dd.ids = cs.dyn_ids.p;
	dd.n_padded = cs.dyn_padded;
	return dd;
}

// ---- lmx_capi_cull_set.hip ------------------------------------------------------------------------------------------------------
void queue_dyn_patch(CullSet& cs, const DynRec& r, bool alive);
void fold_overflow(CullSet& cs); // move the unbound part of the dynamic set back into the static mirror
int async_replay(LmxContext* ctx, CullSet& cs, const CullOp* ops, size_t n); // logged operations onto the shadow set (next to the _impl functions it calls)

// ---- lmx_capi_cull.hip ----------------------------------------------------------------------------------------------------------
extern std::atomic<uint64_t> g_layout_generation;
int apply_patches_on(LmxContext* ctx, CullSet& cs, hipStream_t stream, bool profile);
int rebuild_static_on(LmxContext* ctx, CullSet& cs, hipStream_t stream, uint32_t overflow_reserve, PinnedUploader* up = nullptr);
int rebuild_dynamic_on(LmxContext* ctx, CullSet& cs, hipStream_t stream, uint32_t overflow_reserve, PinnedUploader* up = nullptr);
int recompute_out_layout(LmxContext* ctx);
bool wants_compaction(const CullState& cs);

// ---- lmx_capi_cull_async.hip: its only entrances ---------------------------------------------------------------------------------
int async_enable(LmxContext* ctx);
void async_disable(CullState& cs);
int async_poll(LmxContext* ctx, bool* swapped); // from the flush of a live layout
void async_reseed(CullState& cs);               // after a synchronous compaction
void async_wait_idle(CullAsync& a);

} // namespace lmx
