// texcomp_kernels.hip — the texture compressor (TextureCompressor::compress's per-block loops, renderer/editor/render_plugins.cpp:226,261,291)
// on the device. The arithmetic is lmx_texcomp.h's, shared with the host; FMA-free (-ffp-contract=off). The kernels need no scratch buffers.
//
//   k_bc4         one lane per (block, channel): BC4 of one channel, BC5 as channels 0 and 1, BC3's alpha half as channel 3.
//   k_bc1_search  ONE WAVE per 4 x 4 block, TC_WAVES blocks per workgroup, a grid stride over the blocks. Lane l reads texel l & 15; the sixteen
//                 pixels then go to every lane by readlane, so what stands before the search (totals, initial endpoints, up to two
//                 least-squares passes, their selectors and error) is computed by all lanes alike from wave-uniform values. The sort along
//                 the endpoint axis is a rank per pixel (sixteen compares in the pixel's lane); lane k <= 16 then adds the pixels of rank
//                 below k: the prefix sums r_sum / g_sum / b_sum[k] live in lane k and a trial reads its three places by a shuffle.
//                 The 969 histograms are strided over the 64 lanes, 16 rounds; their table and the midpoints are staged in LDS once per
//                 workgroup. A lane keeps the least `err << 10 | index` of its trials, a butterfly of __shfl_xor takes the wave's minimum,
//                 and every lane recomputes the winner (its endpoints and selectors are wave-uniform again). With 3-colour blocks allowed
//                 the same wave runs try_3color_block the same way over the 153 histograms. Lane 0 writes the eight bytes.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "lmx_texcomp.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

static_assert(offsetof(TcTables, match) == TC_LDS_WORDS * 4, "the histograms and the midpoints are the head of TcTables");
static_assert(sizeof(TcHist) == 16, "a histogram is one 16-byte LDS read");

__global__ __launch_bounds__(TC_BLOCK) void k_bc4(TcBatch batch, uint32_t n_channels, uint32_t shift0, uint32_t shift1, uint32_t* __restrict__ out, uint32_t stride_words) {
	const uint32_t t = blockIdx.x * TC_BLOCK + threadIdx.x;
	const uint32_t b = t / n_channels, ch = t % n_channels;
	if (b >= batch.n_blocks) return;
	const TcImage im = batch.images[tc_image_of(batch.images, batch.n_images, b)];
	uint32_t px[16];
#pragma unroll
	for (uint32_t i = 0; i < 16; ++i) px[i] = tc_texel(im, batch.rgba, b, i);
	const TcBlock blk = tc_encode_bc4(px, ch == 0 ? shift0 : shift1);
	*reinterpret_cast<uint2*>(out + (size_t)b * stride_words + 2 * ch) = make_uint2(blk.w0, blk.w1);
}

// the wave's minimum of a key, in every lane
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t o = __shfl_xor(v, off);
		v = o < v ? o : v;
	}
	return v;
}

// The prefix sums of the block sorted along the axis of `e`: lane k <= 16 gets the sums of the k pixels of lowest key, r | g << 16 and b.
// `mine` is the lane's own pixel (texel lane & 15), px the sixteen pixels (wave-uniform).
__device__ __forceinline__ void sorted_sums(const uint32_t px[16], uint32_t mine, uint32_t lane, const TcEnd& e, uint32_t* sum_rg, uint32_t* sum_b) {
	const TcAxis a = tc_axis(e);
	const int my_key = tc_sort_key(mine, a, (int)(lane & 15u));
	uint32_t rank = 0;
#pragma unroll
	for (int j = 0; j < 16; ++j) rank += tc_sort_key(px[j], a, j) < my_key ? 1u : 0u;
	uint32_t rg = 0, bb = 0;
#pragma unroll
	for (int j = 0; j < 16; ++j) {
		const uint32_t rank_j = (uint32_t)__builtin_amdgcn_readlane((int)rank, j);
		if (rank_j < lane) {
			rg += tc_r(px[j]) | tc_g(px[j]) << 16;
			bb += tc_b(px[j]);
		}
	}
	*sum_rg = rg;
	*sum_b = bb;
}

// trial `q` of the wave's block: every lane calls it (the sums come by shuffles), each with its own q
__device__ __forceinline__ uint32_t trial_of(bool four, const uint32_t px[16], const TcTotals& t, const TcHist& h, uint32_t sum_rg, uint32_t sum_b, const float* mid5, const float* mid6,
	const uint32_t* match, TcEnd* e, uint32_t* sels) {
	const int f1 = (int)(h.f & 255u), f2 = (int)((h.f >> 8) & 255u), f3 = (int)((h.f >> 16) & 255u);
	const uint32_t rg1 = __shfl(sum_rg, f1), b1 = __shfl(sum_b, f1), rg2 = __shfl(sum_rg, f2), b2 = __shfl(sum_b, f2);
	uint32_t rg3 = 0, b3 = 0;
	if (four) { // (compile-time)
		rg3 = __shfl(sum_rg, f3);
		b3 = __shfl(sum_b, f3);
	}
	const uint32_t s1[3] = {rg1 & 0xffffu, rg1 >> 16, b1}, s2[3] = {rg2 & 0xffffu, rg2 >> 16, b2}, s3[3] = {rg3 & 0xffffu, rg3 >> 16, b3};
	return tc_trial(four, px, t, h, s1, s2, s3, mid5, mid6, match, e, sels);
}

// the search over all histograms behind state `st` (wave-uniform in, wave-uniform out)
template <bool FOUR>
__device__ __forceinline__ void search(const uint32_t px[16], uint32_t mine, uint32_t lane, const TcTotals& t, const TcHist* hist, const float* mid5, const float* mid6, const uint32_t* match,
	TcState* st) {
	constexpr uint32_t N = FOUR ? TC_HIST4 : TC_HIST3;
	uint32_t sum_rg, sum_b;
	sorted_sums(px, mine, lane, st->e, &sum_rg, &sum_b);
	uint32_t best = 0xffffffffu;
#pragma unroll 1
	for (uint32_t base = 0; base < N; base += 64) { // (wave-uniform trip count: the shuffles inside want every lane)
		const uint32_t q = base + lane;
		const TcHist h = hist[q < N ? q : 0];
		TcEnd e;
		uint32_t sels;
		const uint32_t err = trial_of(FOUR, px, t, h, sum_rg, sum_b, mid5, mid6, match, &e, &sels);
		const uint32_t key = q < N ? tc_trial_key(err, q) : 0xffffffffu;
		best = key < best ? key : best;
	}
	best = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_min(best));
	if ((best >> 10) < st->err) { // strictly better only; the winner again, now in every lane
		const TcHist h = hist[best & 1023u];
		st->err = trial_of(FOUR, px, t, h, sum_rg, sum_b, mid5, mid6, match, &st->e, &st->sels);
	}
}

// (four waves per SIMD asked for: the largest grid, TC_MAX_GRID workgroups, is then resident at once, so no workgroup of equal work starts late)
template <bool ALLOW3>
__global__ __launch_bounds__(TC_BLOCK, TC_WAVES_PER_SIMD) void k_bc1_search(TcBatch batch, const TcTables* __restrict__ tables, uint32_t* __restrict__ out, uint32_t stride_words, uint32_t at_word) {
	__shared__ uint32_t s_tab[TC_LDS_WORDS];
	{
		const uint32_t* src = reinterpret_cast<const uint32_t*>(tables);
		for (uint32_t k = threadIdx.x; k < TC_LDS_WORDS; k += TC_BLOCK) s_tab[k] = src[k];
	}
	__syncthreads();
	const TcHist* hist4 = reinterpret_cast<const TcHist*>(s_tab);
	const TcHist* hist3 = hist4 + TC_HIST4;
	const float* mid5 = reinterpret_cast<const float*>(hist3 + TC_HIST3);
	const float* mid6 = mid5 + 32;
	const uint32_t* match = &tables->match[0][0];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll 1
	for (uint32_t b = blockIdx.x * TC_WAVES + wave; b < batch.n_blocks; b += gridDim.x * TC_WAVES) { // (no barrier inside: waves leave on their own)
		const TcImage im = batch.images[tc_image_of(batch.images, batch.n_images, b)];
		const uint32_t mine = tc_texel(im, batch.rgba, b, lane & 15u);
		uint32_t px[16];
#pragma unroll
		for (int i = 0; i < 16; ++i) px[i] = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
		TcBlock blk;
		if (tc_solid(px)) blk = tc_solid_block(tc_r(px[0]), tc_g(px[0]), tc_b(px[0]), ALLOW3, match);
		else {
			const TcTotals t = tc_totals(px);
			const TcEnd first = tc_pick_initial(px, t);
			TcState s4 = tc_refine(true, px, t, first, mid5, mid6, match);
			if (s4.err) search<true>(px, mine, lane, t, hist4, mid5, mid6, match, &s4);
			bool three = false;
			TcState s3 = s4;
			if (ALLOW3 && s4.err) {
				s3 = tc_refine(false, px, t, first, mid5, mid6, match);
				if (s3.err) search<false>(px, mine, lane, t, hist3, mid5, mid6, match, &s3);
				three = s3.err < s4.err;
			}
			blk = three ? tc_encode3(s3.e, s3.sels) : tc_encode4(s4.e, s4.sels);
		}
		if (lane == 0) *reinterpret_cast<uint2*>(out + (size_t)b * stride_words + at_word) = make_uint2(blk.w0, blk.w1);
	}
}

bool batch_ok(const TcBatch& b) { return b.images && b.rgba && b.n_images != 0 && b.n_blocks != 0; }

} // namespace

hipError_t launch_bc1_search(hipStream_t s, const TcBatch& batch, const TcTables* tables, bool allow_3color, uint32_t* out, uint32_t stride_words, uint32_t at_word) {
	if (!batch_ok(batch) || !tables || !out || (stride_words != 2 && stride_words != 4) || at_word + 2 > stride_words || (at_word & 1u)) return hipErrorInvalidValue;
	const uint32_t want = (batch.n_blocks + TC_WAVES - 1) / TC_WAVES;
	const uint32_t grid = want < TC_MAX_GRID ? want : TC_MAX_GRID;
	if (allow_3color) hipLaunchKernelGGL(k_bc1_search<true>, dim3(grid), dim3(TC_BLOCK), 0, s, batch, tables, out, stride_words, at_word);
	else hipLaunchKernelGGL(k_bc1_search<false>, dim3(grid), dim3(TC_BLOCK), 0, s, batch, tables, out, stride_words, at_word);
	return hipGetLastError();
}

hipError_t launch_bc4(hipStream_t s, const TcBatch& batch, uint32_t n_channels, uint32_t shift0, uint32_t shift1, uint32_t* out, uint32_t stride_words) {
	if (!batch_ok(batch) || !out || n_channels == 0 || n_channels > 2 || stride_words < 2 * n_channels || shift0 > 24 || shift1 > 24) return hipErrorInvalidValue;
	const uint64_t lanes = (uint64_t)batch.n_blocks * n_channels;
	hipLaunchKernelGGL(k_bc4, dim3((uint32_t)((lanes + TC_BLOCK - 1) / TC_BLOCK)), dim3(TC_BLOCK), 0, s, batch, n_channels, shift0, shift1, out, stride_words);
	return hipGetLastError();
}

} // namespace lmx
