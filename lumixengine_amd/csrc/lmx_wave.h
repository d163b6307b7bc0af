// lmx_wave.h — the kernels' wave64 and block vocabulary for ranks, scans and appends. Device-only, header-only; a new kernel takes its
// scans and appends from here ("Wave and block vocabulary"). tests/hostsim/selftest.cpp checks every function below against a
// sequential fold on the host.
//
// Blocks are one-dimensional: a thread's place is threadIdx.x, its wave threadIdx.x >> 6, its lane threadIdx.x & 63.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lmx {

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// the bits of `mask` below this lane: the lane's rank among the lanes of a ballot
__device__ __forceinline__ uint32_t rank_in(uint64_t mask) {
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t mbcnt64(uint64_t mask) { return rank_in(mask); } // (the cull kernels' spelling)

// a + b, held at 2^32 - 1
__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) {
	const uint32_t s = a + b;
	return s < a ? 0xffffffffu : s;
}

// the scans' operators: op(earlier, later), associative, not necessarily commutative
struct Sum {
	__device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct SatAdd {
	__device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return sat_add(a, b); }
};

// Inclusive scan over the wave in lane order: lane l gets op(v[0], ... v[l]). Every lane of the wave is active; `lane` is this lane's
// index as the caller already holds it (lane_id() or threadIdx.x & 63).
template <typename Op> __device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, uint32_t lane, Op op) {
#pragma unroll
	for (uint32_t off = 1; off < 64; off <<= 1) {
		const uint32_t up = __shfl_up(v, off);
		if (lane >= off) v = op(up, v);
	}
	return v;
}
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) { return wave_inclusive(v, lane, Sum()); }

// Scan over the block in thread order; *total = the fold of the whole block, in every thread.
//   - Every thread of the block calls it, under block-uniform control flow (two barriers inside); n_waves = blockDim.x / 64.
//   - s_wave holds n_waves words of LDS and is free again on return (the trailing barrier): the next call may use the same words.
//   - EXCLUSIVE: a thread gets the INCLUSIVE value of the thread before it, and the block's first thread gets `identity`. Nothing is
//     ever taken back out of a value, so saturating sums (v - own would be wrong once the sum is held at 2^32 - 1) and operators
//     without an inverse (composition of maps) come out right.
//   - `identity` is op's neutral element: 0 for the sums, the identity map for a composition.
template <bool EXCLUSIVE, typename Op> __device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t n_waves, uint32_t identity, uint32_t* s_wave, uint32_t* total, Op op) {
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	v = wave_inclusive(v, lane, op);
	if (lane == 63) s_wave[wave] = v;
	if (EXCLUSIVE) {
		v = __shfl_up(v, 1u);
		if (lane == 0) v = identity;
	}
	__syncthreads();
	uint32_t pre = identity, all = identity;
	for (uint32_t w = 0; w < n_waves; ++w) {
		const uint32_t sw = s_wave[w];
		if (w < wave) pre = op(pre, sw);
		all = op(all, sw);
	}
	__syncthreads();
	*total = all;
	return op(pre, v);
}

// Wave-aggregated append to a list whose length lives at *counter (uint32_t or unsigned long long): every lane with `want` gets a
// distinct index; the value is meaningless where !want. One returning atomic per wave, none when no active lane wants. Works under
// divergence: the leader is the first wanting lane of the ballot, which is an active one.
template <typename Counter> __device__ __forceinline__ Counter wave_append(bool want, Counter* counter) {
	const uint64_t mask = __ballot(want);
	if (mask == 0) return 0;
	Counter base = 0;
	const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
	if (lane_id() == leader) base = atomicAdd(counter, (Counter)__popcll(mask));
	base = __shfl(base, (int)leader);
	return base + rank_in(mask);
}

// the length of a device-side list as the kernels see it: the producer's counter may have run past the capacity
__device__ __forceinline__ uint32_t device_count(const uint32_t* count, uint32_t cap) {
	const uint32_t n = *count;
	return n < cap ? n : cap;
}
// ... of the list a pass was handed: `D` is the pass's device struct, which carries list_count / list_cap under these names
template <typename D> __device__ __forceinline__ uint32_t list_length(const D& d) { return device_count(d.list_count, d.list_cap); }

} // namespace lmx
