// selftest.cpp — TEST INFRASTRUCTURE: pins the simulated device's semantics (tests/hostsim) on kernels whose results are known by
// construction: wave64 ballots and ranks, readlane / readfirstlane under divergence, shuffles, DPP quad permutes, LDS exchange behind
// the block barrier and the wave barrier, early-exit loops (lanes that left a loop wait for the others at the reconvergence point),
// dynamic LDS, the kernarg segment, atomics. Exit code 0 = all good.
//
// The second half checks the kernels' own wave / block vocabulary (lumixengine_amd/csrc/lmx_wave.h) against a sequential fold on the
// host: wave_inclusive, block_scan in both forms (sum, saturating sum, a non-commutative composition), wave_append.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "lmx_wave.h"

namespace {

using lmx::lane_id;
using lmx::mbcnt64;

// out[tid]: [0] ballot of (lane % 3 == 0) low word, [1] rank among them, [2] ballot inside a divergent branch (odd lanes), [3] readfirstlane in that branch,
// [4] full ballot after the branch
__global__ void k_ballots(uint32_t* out) {
	const uint32_t lane = lane_id(), t = threadIdx.x;
	const uint64_t m = __ballot(lane % 3u == 0u);
	out[5 * t + 0] = (uint32_t)m ^ (uint32_t)(m >> 32);
	out[5 * t + 1] = mbcnt64(m);
	uint32_t inner = 0, first = 0;
	if (lane & 1u) {
		inner = (uint32_t)__popcll(__ballot(lane < 40u)); // only odd lanes are active: 20 of them are below 40
		first = __builtin_amdgcn_readfirstlane(lane * 7u); // lowest active lane is lane 1
	}
	out[5 * t + 2] = inner;
	out[5 * t + 3] = first;
	out[5 * t + 4] = (uint32_t)__popcll(__ballot(true));
}

// lanes leave the loop after (lane % 5) + 1 iterations; each iteration holds a ballot of the lanes still looping
__global__ void k_loop(uint32_t* out) {
	const uint32_t lane = lane_id();
	uint32_t acc = 0;
	for (uint32_t it = 0; it <= lane % 5u; ++it) acc += (uint32_t)__popcll(__ballot(true)); // lanes with lane % 5 >= it
	const uint32_t after = (uint32_t)__popcll(__ballot(true));                                 // all 64 again
	out[2 * threadIdx.x] = acc;
	out[2 * threadIdx.x + 1] = after;
}

__global__ void k_shuffles(int* out) {
	const int lane = (int)lane_id();
	const int v = 100 + lane;
	int* o = out + 6 * threadIdx.x;
	o[0] = __shfl(v, 5);
	o[1] = __shfl_up(v, 3);
	o[2] = __shfl_down(v, 4);
	o[3] = __shfl_xor(v, 32);
	o[4] = __builtin_amdgcn_readlane(v, 63);
	o[5] = __builtin_amdgcn_mov_dpp(v, 1 | 2 << 2 | 3 << 4 | 3 << 6, 0xf, 0xf, true); // quad_perm [1, 2, 3, 3]
}

// block of 256: reverse through static LDS behind the block barrier, rotate inside the wave through LDS behind the wave barrier,
// dynamic LDS carries a per-wave sum, the kernarg segment is read directly
struct Args { uint32_t magic[4]; };
__global__ void k_lds(const Args a, const uint32_t* in, uint32_t* out, uint32_t* counter) {
	__shared__ uint32_t s_a[256];
	__shared__ uint32_t s_b[256];
	LMX_DYNAMIC_LDS(uint32_t, s_dyn);
	const uint32_t t = threadIdx.x, lane = lane_id(), wave = t >> 6;
	s_a[t] = in[blockIdx.x * 256u + t];
	if (t < 4) s_dyn[t] = 0;
	__syncthreads();
	const uint32_t rev = s_a[255u - t];
	s_b[t] = rev;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	const uint32_t rot = s_b[wave * 64u + ((lane + 1u) & 63u)];
	atomicAdd(&s_dyn[wave], rot);
	__syncthreads();
	const uint32_t* ka = (const uint32_t*)__builtin_amdgcn_kernarg_segment_ptr();
	out[blockIdx.x * 256u + t] = rot + ka[lane & 3u] + s_dyn[wave] * 0u + (a.magic[0] - ka[0]);
	if (lane == 0) atomicAdd(counter, s_dyn[wave]);
}

// ---- lmx_wave.h ------------------------------------------------------------------------------------------------------------------
// The non-commutative operator: maps {0..3} -> {0..3}, two bits per entry (the draw pass's state maps); "first f, then g".
constexpr uint32_t MAP_IDENTITY = 0xE4u;
struct Compose {
	__host__ __device__ uint32_t operator()(uint32_t f, uint32_t g) const {
		uint32_t r = 0;
		for (uint32_t s = 0; s < 4; ++s) r |= ((g >> (2 * ((f >> (2 * s)) & 3u))) & 3u) << (2 * s);
		return r;
	}
};
struct HostSum {
	uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct HostSatAdd {
	uint32_t operator()(uint32_t a, uint32_t b) const { return a + b < a ? 0xffffffffu : a + b; }
};

// out[lane] = the inclusive sum of lane + 1, out[64 + lane] = the inclusive composition of in[0 .. lane]
__global__ void k_wave_scan(const uint32_t* in, uint32_t* out) {
	const uint32_t lane = lane_id();
	out[lane] = lmx::wave_inclusive_sum(lane + 1u, lane);
	out[64u + lane] = lmx::wave_inclusive(in[lane], lane, Compose());
}

// Two scans back to back over ONE s_wave: the block's n inputs in thread order, then the same inputs in reverse order.
// out: [2][blocks][n] scan values, then [2][blocks][2] totals as thread 0 and as the last thread got them.
template <bool EXCLUSIVE, typename Op> __global__ void k_block_scan(const uint32_t* in, uint32_t identity, uint32_t* out) {
	__shared__ uint32_t s_wave[16];
	const uint32_t n = blockDim.x, t = threadIdx.x, b = blockIdx.x, blocks = gridDim.x;
	uint32_t total[2];
	out[b * n + t] = lmx::block_scan<EXCLUSIVE>(in[b * n + t], n >> 6, identity, s_wave, &total[0], Op());
	out[(blocks + b) * n + t] = lmx::block_scan<EXCLUSIVE>(in[b * n + (n - 1u - t)], n >> 6, identity, s_wave, &total[1], Op());
	uint32_t* totals = out + 2u * blocks * n;
	for (uint32_t c = 0; c < 2; ++c) {
		if (t == 0) totals[(c * blocks + b) * 2u] = total[c];
		if (t == n - 1u) totals[(c * blocks + b) * 2u + 1u] = total[c];
	}
}

// out[thread] = the index the thread got, or all ones where it did not want one
enum { APPEND_NONE, APPEND_LANE_63, APPEND_ALL, APPEND_ODD_DIVERGENT };
template <typename Counter> __global__ void k_append(uint32_t mode, Counter* counter, Counter* out) {
	const uint32_t lane = lane_id();
	Counter idx = ~(Counter)0;
	if (mode == APPEND_ODD_DIVERGENT) {
		if (lane & 1u) idx = lmx::wave_append(true, counter); // the even lanes are not here: the leader is lane 1
	} else {
		const bool want = mode == APPEND_ALL || (mode == APPEND_LANE_63 && lane == 63u);
		const Counter got = lmx::wave_append(want, counter);
		if (want) idx = got;
	}
	out[threadIdx.x] = idx;
}

int fails = 0;
void check(bool ok, const char* what) {
	if (!ok) {
		printf("FAIL: %s\n", what);
		++fails;
	}
}

uint32_t rng_state = 12345u;
uint32_t rng() { // xorshift32
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 17;
	rng_state ^= rng_state << 5;
	return rng_state;
}

// `blocks` blocks of n threads: both forms of block_scan against the sequential fold of the same inputs
template <typename Op, typename HostOp> void check_block_scan(const std::vector<uint32_t>& in, uint32_t blocks, uint32_t n, uint32_t identity, HostOp op, const char* what) {
	const size_t n_out = 2 * (size_t)blocks * n + 4 * (size_t)blocks;
	uint32_t *din, *dout;
	(void)hipMalloc(&din, in.size() * 4);
	(void)hipMalloc(&dout, n_out * 4);
	(void)hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice);
	for (int exclusive = 0; exclusive < 2; ++exclusive) {
		(void)hipMemset(dout, 0xA5, n_out * 4);
		if (exclusive) hipLaunchKernelGGL((k_block_scan<true, Op>), dim3(blocks), dim3(n), 0, 0, din, identity, dout);
		else hipLaunchKernelGGL((k_block_scan<false, Op>), dim3(blocks), dim3(n), 0, 0, din, identity, dout);
		std::vector<uint32_t> out(n_out);
		(void)hipMemcpy(out.data(), dout, n_out * 4, hipMemcpyDeviceToHost);
		bool ok = true;
		for (uint32_t call = 0; call < 2; ++call)
			for (uint32_t b = 0; b < blocks; ++b) {
				uint32_t run = identity;
				for (uint32_t t = 0; t < n; ++t) {
					const uint32_t before = run;
					run = op(run, in[b * n + (call ? n - 1u - t : t)]);
					ok &= out[(call * blocks + b) * n + t] == (exclusive ? before : run);
				}
				const uint32_t* totals = &out[2 * (size_t)blocks * n + (call * blocks + b) * 2];
				ok &= totals[0] == run && totals[1] == run;
			}
		if (!ok) printf("  (%s, %u threads, %s)\n", what, n, exclusive ? "exclusive" : "inclusive");
		check(ok, "block_scan against the sequential fold");
	}
	(void)hipFree(din);
	(void)hipFree(dout);
}

// one block of n_threads on a counter that starts at `start`: the wanting threads' indices are start .. start + n_want - 1, each once -
// inside a wave in lane order - and the counter ends at start + n_want
template <typename Counter> void check_append(uint32_t mode, uint32_t n_threads, Counter start, uint32_t n_want, const char* what) {
	Counter *dcnt, *dout;
	(void)hipMalloc(&dcnt, sizeof(Counter));
	(void)hipMalloc(&dout, n_threads * sizeof(Counter));
	(void)hipMemcpy(dcnt, &start, sizeof(Counter), hipMemcpyHostToDevice);
	hipLaunchKernelGGL((k_append<Counter>), dim3(1), dim3(n_threads), 0, 0, mode, dcnt, dout);
	std::vector<Counter> out(n_threads);
	Counter end = 0;
	(void)hipMemcpy(out.data(), dout, n_threads * sizeof(Counter), hipMemcpyDeviceToHost);
	(void)hipMemcpy(&end, dcnt, sizeof(Counter), hipMemcpyDeviceToHost);
	bool ok = end == start + n_want;
	std::vector<Counter> got;
	int prev_wave = -1;
	for (uint32_t t = 0; t < n_threads; ++t) {
		const uint32_t lane = t & 63u;
		const bool wants = mode == APPEND_ALL || (mode == APPEND_LANE_63 && lane == 63u) || (mode == APPEND_ODD_DIVERGENT && (lane & 1u));
		ok &= wants == (out[t] != ~(Counter)0);
		if (!wants) continue;
		if (prev_wave == (int)(t >> 6)) ok &= out[t] == got.back() + 1; // behind the wanting lane before it in the same wave
		prev_wave = (int)(t >> 6);
		got.push_back(out[t]);
	}
	std::sort(got.begin(), got.end());
	ok &= got.size() == n_want;
	for (size_t i = 0; i < got.size(); ++i) ok &= got[i] == start + (Counter)i;
	check(ok, what);
	(void)hipFree(dcnt);
	(void)hipFree(dout);
}

} // namespace

int main() {
	{
		uint32_t* d;
		(void)hipMalloc(&d, 128 * 5 * 4);
		hipLaunchKernelGGL(k_ballots, dim3(1), dim3(128), 0, 0, d);
		std::vector<uint32_t> h(128 * 5);
		(void)hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost);
		uint64_t m = 0;
		for (int l = 0; l < 64; ++l) if (l % 3 == 0) m |= 1ull << l;
		bool ok = true;
		for (int t = 0; t < 128; ++t) {
			const int l = t & 63;
			ok &= h[5 * t] == ((uint32_t)m ^ (uint32_t)(m >> 32));
			ok &= h[5 * t + 1] == (uint32_t)__builtin_popcountll(m & ((1ull << l) - 1));
			ok &= h[5 * t + 2] == ((l & 1) ? 20u : 0u);
			ok &= h[5 * t + 3] == ((l & 1) ? 7u : 0u);
			ok &= h[5 * t + 4] == 64u;
		}
		check(ok, "ballot / mbcnt / divergent ballot / readfirstlane");
		(void)hipFree(d);
	}
	{
		uint32_t* d;
		(void)hipMalloc(&d, 64 * 2 * 4);
		hipLaunchKernelGGL(k_loop, dim3(1), dim3(64), 0, 0, d);
		std::vector<uint32_t> h(128);
		(void)hipMemcpy(h.data(), d, 512, hipMemcpyDeviceToHost);
		bool ok = true;
		uint32_t still[5];
		for (int it = 0; it < 5; ++it) {
			still[it] = 0;
			for (int l = 0; l < 64; ++l) still[it] += (l % 5 >= it);
		}
		for (int l = 0; l < 64; ++l) {
			uint32_t want = 0;
			for (int it = 0; it <= l % 5; ++it) want += still[it];
			ok &= h[2 * l] == want && h[2 * l + 1] == 64u;
		}
		check(ok, "early-exit loop: per-iteration EXEC masks and reconvergence behind the loop");
		(void)hipFree(d);
	}
	{
		int* d;
		(void)hipMalloc(&d, 64 * 6 * 4);
		hipLaunchKernelGGL(k_shuffles, dim3(1), dim3(64), 0, 0, d);
		std::vector<int> h(64 * 6);
		(void)hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost);
		bool ok = true;
		const int perm[4] = {1, 2, 3, 3};
		for (int l = 0; l < 64; ++l) {
			const int* o = &h[6 * l];
			ok &= o[0] == 105;
			ok &= o[1] == (l >= 3 ? 100 + l - 3 : 100 + l);
			ok &= o[2] == (l + 4 < 64 ? 100 + l + 4 : 100 + l);
			ok &= o[3] == 100 + (l ^ 32);
			ok &= o[4] == 163;
			ok &= o[5] == 100 + (l & ~3) + perm[l & 3];
		}
		check(ok, "shuffles / readlane / DPP quad_perm");
		(void)hipFree(d);
	}
	{
		const uint32_t blocks = 7;
		std::vector<uint32_t> in(blocks * 256), out(blocks * 256);
		for (size_t i = 0; i < in.size(); ++i) in[i] = (uint32_t)(i * 2654435761u);
		uint32_t *din, *dout, *dcnt;
		(void)hipMalloc(&din, in.size() * 4);
		(void)hipMalloc(&dout, in.size() * 4);
		(void)hipMalloc(&dcnt, 4);
		(void)hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice);
		(void)hipMemset(dcnt, 0, 4);
		Args a = {{11, 22, 33, 44}};
		hipLaunchKernelGGL(k_lds, dim3(blocks), dim3(256), 16, 0, a, din, dout, dcnt);
		check(hipGetLastError() == hipSuccess, "launch");
		(void)hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost);
		uint32_t cnt = 0, want_cnt = 0;
		(void)hipMemcpy(&cnt, dcnt, 4, hipMemcpyDeviceToHost);
		bool ok = true;
		for (uint32_t b = 0; b < blocks; ++b)
			for (uint32_t t = 0; t < 256; ++t) {
				const uint32_t wave = t >> 6, lane = t & 63u;
				const uint32_t src = wave * 64u + ((lane + 1u) & 63u); // index into the reversed array
				const uint32_t rot = in[b * 256u + 255u - src];
				ok &= out[b * 256u + t] == rot + a.magic[lane & 3u];
				want_cnt += rot;
			}
		check(ok, "static LDS / wave barrier / kernarg segment");
		check(cnt == want_cnt, "dynamic LDS + atomics");
		(void)hipFree(din);
		(void)hipFree(dout);
		(void)hipFree(dcnt);
	}
	{ // wave_inclusive: the sum of lane + 1, and the composition (not commutative) of pseudo-random maps
		std::vector<uint32_t> in(64), out(128);
		for (auto& v : in) v = rng() & 0xffu;
		uint32_t *din, *dout;
		(void)hipMalloc(&din, 64 * 4);
		(void)hipMalloc(&dout, 128 * 4);
		(void)hipMemcpy(din, in.data(), 64 * 4, hipMemcpyHostToDevice);
		hipLaunchKernelGGL(k_wave_scan, dim3(1), dim3(64), 0, 0, din, dout);
		(void)hipMemcpy(out.data(), dout, 128 * 4, hipMemcpyDeviceToHost);
		bool ok = true;
		uint32_t run = MAP_IDENTITY;
		for (uint32_t l = 0; l < 64; ++l) {
			run = Compose()(run, in[l]);
			ok &= out[l] == (l + 1) * (l + 2) / 2 && out[64 + l] == run;
		}
		check(ok, "wave_inclusive: sum and non-commutative composition");
		check(Compose()(0x00u, 0xFFu) == 0xFFu && Compose()(0xFFu, 0x00u) == 0x00u, "the composition used here does not commute"); // (two constant maps)
		(void)hipFree(din);
		(void)hipFree(dout);
	}
	for (uint32_t n : {64u, 256u, 1024u}) { // block_scan, two blocks of pseudo-random inputs: the wrapping sum and the composition
		std::vector<uint32_t> words(2 * n), maps(2 * n);
		for (auto& v : words) v = rng();
		for (auto& v : maps) v = rng() & 0xffu;
		check_block_scan<lmx::Sum>(words, 2, n, 0u, HostSum(), "sum");
		check_block_scan<Compose>(maps, 2, n, MAP_IDENTITY, Compose(), "composition"); // (exclusive: thread 0 of a block gets MAP_IDENTITY, not 0)
		// The saturating sum, one block per place where the running sum reaches 2^32 - 1: thread `tip` is the first whose inclusive value
		// is held there (the values before it add up to 2^32 - 2, its own is >= 2), and every value behind it is > 0, so that an
		// exclusive value formed as "inclusive - own" would come out wrong everywhere behind the tip.
		//   inside a wave | exactly between lane 63 of wave 0 and lane 0 of wave 1 (blocks of more than one wave) | only in the block's total
		std::vector<uint32_t> tips = {37u, n - 1u};
		if (n > 64u) tips.insert(tips.begin() + 1, 64u);
		std::vector<uint32_t> sat(tips.size() * n);
		for (size_t b = 0; b < tips.size(); ++b) {
			uint32_t* v = &sat[b * n];
			uint32_t before = 0;
			for (uint32_t t = 0; t < n; ++t) {
				v[t] = 2u + rng() % 999u;
				if (t >= 1 && t < tips[b]) before += v[t];
			}
			v[0] = 0xfffffffeu - before;
		}
		check_block_scan<lmx::SatAdd>(sat, (uint32_t)tips.size(), n, 0u, HostSatAdd(), "saturating sum");
	}
	// wave_append
	check_append<uint32_t>(APPEND_NONE, 64, 7u, 0, "wave_append: nobody wants - the counter is unchanged");
	check_append<uint32_t>(APPEND_LANE_63, 64, 7u, 1, "wave_append: only lane 63 wants");
	check_append<uint32_t>(APPEND_ALL, 64, 7u, 64, "wave_append: all 64 lanes want");
	check_append<uint32_t>(APPEND_ODD_DIVERGENT, 64, 7u, 32, "wave_append: the odd lanes, inside a divergent branch");
	check_append<uint32_t>(APPEND_ALL, 128, 0u, 128, "wave_append: two waves on one counter - a permutation of 0 .. n - 1");
	check_append<unsigned long long>(APPEND_ALL, 64, 0xfffffffdull, 64, "wave_append: the 64-bit counter carries past 2^32");
	printf(fails ? "hostsim selftest: %d failure(s)\n" : "hostsim selftest: ok\n", fails);
	return fails ? 1 : 0;
}
