// texmips_kernels.hip — a texture's mip chain on the device (TextureCompressor::compress with generate_mipmaps, renderer/editor/
// render_plugins.cpp:359-401: computeMip, computeCoverage, scaleCoverage). The arithmetic is lmx_texmips.h's, shared with the host; FMA-free
// (-ffp-contract=off). No kernel uses scratch: the taps are read from LDS where they are indexed at run time.
//
//   k_mip_level<mode>  one level of every chain of the batch in one launch; blockIdx.y is the chain.
//                      Filtered modes: a workgroup makes one TM_TILE x TM_TILE tile of output texels. It stages the taps of its 16 columns and
//                      16 rows, and the source window they reach (n0 of the first output to the last texel of any) as RGBA8 words in LDS;
//                      runs the horizontal pass into seven planes of floats per (window row, output column); behind a barrier runs the
//                      vertical pass with one lane per output texel, encodes and stores 4 bytes per lane, 16 lanes to 64 contiguous bytes.
//                      Stochastic mode: one lane per output texel, the generator entered at draw 2 i of row j by voxel_rng_skip; no window.
//                      With coverage on, the alpha histogram of the level written is gathered in the same launch: LDS bins per workgroup,
//                      then one atomic add per non-empty bin into the chain's 256 global bins.
//   k_mip_scale        every workgroup re-derives scaleCoverage's factor from the level's histogram (wave-uniform, at most 255 steps over
//                      LDS) and rescales the alpha of its texels in place.
//   k_mip_tail<mode>   once both sides of a level are at most 32, one workgroup per chain makes all levels behind it in LDS with barriers in
//                      between, histogram and rescale included: a 4096 x 4096 chain is 7 level launches and one tail, not 12.
//   k_mip_coverage     computeCoverage's count over the first chain's level 0; k_mip_scale forms the float from it, so no host wait stands
//                      between the set and the blocks.
#include <hip/hip_runtime.h>

#include "lmx_texmips.h"

namespace lmx {

namespace {

template <int MODE> __global__ __launch_bounds__(TM_BLOCK) void k_mip_level(TmLevel L) {
	__shared__ uint32_t s_hist[256];
	const uint32_t tid = threadIdx.x, img = blockIdx.y;
	const uint32_t* __restrict__ src = L.chains + (size_t)img * L.chain_px + L.src_at;
	uint32_t* __restrict__ dst = L.chains + (size_t)img * L.chain_px + L.dst_at;
	s_hist[tid] = 0;
	if constexpr (MODE == TM_STOCHASTIC) {
		__syncthreads();
		const uint32_t t = blockIdx.x * TM_BLOCK + tid;
		if (t < L.dst_w * L.dst_h) {
			const uint32_t px = src[tm_stochastic_pick(L.w, L.h, L.dst_w, L.dst_h, t % L.dst_w, t / L.dst_w)];
			dst[t] = px;
			if (L.histogram) atomicAdd(&s_hist[px >> 24], 1u);
		}
	} else {
		__shared__ uint32_t s_src[TM_WINDOW * TM_WINDOW];
		__shared__ float s_h[7][TM_WINDOW][TM_TILE];
		__shared__ TmRow s_rx[TM_TILE], s_ry[TM_TILE];
		__shared__ float s_tab[512]; // sRGB: the decode table, then the encode table
		const uint32_t tiles_x = (L.dst_w + TM_TILE - 1) / TM_TILE;
		const uint32_t ox0 = (blockIdx.x % tiles_x) * TM_TILE, oy0 = (blockIdx.x / tiles_x) * TM_TILE;
		if (oy0 >= L.dst_h) return; // (block-uniform; the launcher's grid holds no such tile)
		const uint32_t tw = L.dst_w - ox0 < TM_TILE ? L.dst_w - ox0 : TM_TILE, th = L.dst_h - oy0 < TM_TILE ? L.dst_h - oy0 : TM_TILE;
		if (tid < TM_TILE) s_rx[tid] = L.rows_x[ox0 + (tid < tw ? tid : tw - 1)];
		else if (tid < 2 * TM_TILE) s_ry[tid - TM_TILE] = L.rows_y[oy0 + (tid - TM_TILE < th ? tid - TM_TILE : th - 1)];
		if (MODE == TM_SRGB) {
			s_tab[tid] = L.tables->decode[tid];
			s_tab[256 + tid] = L.tables->encode[tid];
		}
		__syncthreads();
		const uint32_t x0 = s_rx[0].n0, y0 = s_ry[0].n0;
		uint32_t x1 = x0, y1 = y0; // one past the last source texel the tile reads
		for (uint32_t k = 0; k < TM_TILE; ++k) {
			const uint32_t xe = s_rx[k].n0 + s_rx[k].n, ye = s_ry[k].n0 + s_ry[k].n;
			x1 = xe > x1 ? xe : x1;
			y1 = ye > y1 ? ye : y1;
		}
		const uint32_t win_w = x1 - x0, win_h = y1 - y0;
		// block-uniform, and never taken: the launcher refuses a level whose tables reach further (tm_max_window) or outside the source
		if (win_w > TM_WINDOW || win_h > TM_WINDOW || x1 > L.w || y1 > L.h) return;
		static_assert(TM_WINDOW <= 64, "a wave stages one window row at a time");
		for (uint32_t r = tid >> 6, c = tid & 63u; r < win_h; r += TM_BLOCK / 64) // (no division by the window's width)
			if (c < win_w) s_src[r * TM_WINDOW + c] = src[(size_t)(y0 + r) * L.w + x0 + c];
		__syncthreads();
		const float* decode = MODE == TM_SRGB ? s_tab : nullptr;
		const float* encode = MODE == TM_SRGB ? s_tab + 256 : nullptr;
		for (uint32_t idx = tid; idx < win_h * TM_TILE; idx += TM_BLOCK) {
			const uint32_t r = idx / TM_TILE, ox = idx % TM_TILE;
			if (ox >= tw) continue;
			const TmRow* row = &s_rx[ox];
			const uint32_t* texel = &s_src[r * TM_WINDOW + (row->n0 - x0)];
			const uint32_t n = row->n < TM_MAX_TAPS ? row->n : TM_MAX_TAPS;
			TmPx acc = tm_zero();
			for (uint32_t k = 0; k < n; ++k) acc = tm_tap(acc, row->c[k], tm_decode(texel[k], decode));
			s_h[0][r][ox] = acc.r;
			s_h[1][r][ox] = acc.g;
			s_h[2][r][ox] = acc.b;
			s_h[3][r][ox] = acc.a;
			s_h[4][r][ox] = acc.ra;
			s_h[5][r][ox] = acc.ga;
			s_h[6][r][ox] = acc.ba;
		}
		__syncthreads();
		const uint32_t ox = tid % TM_TILE, oy = tid / TM_TILE;
		if (ox < tw && oy < th) {
			const TmRow* row = &s_ry[oy];
			const uint32_t r0 = row->n0 - y0;
			const uint32_t n = row->n < TM_MAX_TAPS ? row->n : TM_MAX_TAPS;
			TmPx acc = tm_zero();
			for (uint32_t k = 0; k < n; ++k) {
				const uint32_t r = r0 + k;
				acc = tm_tap(acc, row->c[k], TmPx{s_h[0][r][ox], s_h[1][r][ox], s_h[2][r][ox], s_h[3][r][ox], s_h[4][r][ox], s_h[5][r][ox], s_h[6][r][ox]});
			}
			const uint32_t px = tm_encode(acc, encode);
			dst[(size_t)(oy0 + oy) * L.dst_w + ox0 + ox] = px;
			if (L.histogram) atomicAdd(&s_hist[px >> 24], 1u);
		}
	}
	if (L.histogram) { // (block-uniform)
		__syncthreads();
		const uint32_t mine = s_hist[tid];
		if (mine) atomicAdd(&L.histogram[(size_t)img * 256 + tid], mine);
	}
}

// All levels behind a level of at most TM_TAIL_SIDE x TM_TAIL_SIDE, one workgroup per chain: the level read stays in LDS, every level made
// is at most one 16 x 16 tile and goes to the chain and to LDS, where the next is made from it - after its alpha was rescaled, from the
// workgroup's own 256 LDS bins. The passes are k_mip_level's, sum for sum.
template <int MODE> __global__ __launch_bounds__(TM_BLOCK) void k_mip_tail(TmTail T) {
	__shared__ uint32_t s_px[2][TM_TAIL_SIDE * TM_TAIL_SIDE];
	__shared__ uint32_t s_hist[256];
	__shared__ float s_h[7][TM_TAIL_SIDE][TM_TILE];
	__shared__ float s_tab[512];
	const uint32_t tid = threadIdx.x, ox = tid % TM_TILE, oy = tid / TM_TILE;
	uint32_t* __restrict__ chain = T.chains + (size_t)blockIdx.x * T.chain_px;
	uint32_t w = T.w, h = T.h, at = T.at, cur = 0;
	if (w > TM_TAIL_SIDE || h > TM_TAIL_SIDE) return; // (block-uniform; the launcher refuses it)
	const TmRow* rows = T.rows;
	for (uint32_t idx = tid; idx < w * h; idx += TM_BLOCK) s_px[0][idx] = chain[at + idx];
	if (MODE == TM_SRGB) {
		s_tab[tid] = T.tables->decode[tid];
		s_tab[256 + tid] = T.tables->encode[tid];
	}
	const float* decode = MODE == TM_SRGB ? s_tab : nullptr;
	const float* encode = MODE == TM_SRGB ? s_tab + 256 : nullptr;
	const float wanted = T.count ? tm_coverage(*T.count, T.count_pixels) : 0.0f;
	while (w > 1 || h > 1) { // (block-uniform)
		const uint32_t dw = (w >> 1) ? (w >> 1) : 1u, dh = (h >> 1) ? (h >> 1) : 1u; // at most TM_TILE each
		const bool mine = ox < dw && oy < dh;
		const uint32_t* src = s_px[cur];
		s_hist[tid] = 0;
		__syncthreads(); // the level read is in LDS
		uint32_t px = 0;
		if constexpr (MODE == TM_STOCHASTIC) {
			if (mine) px = src[tm_stochastic_pick(w, h, dw, dh, ox, oy)];
		} else {
			const TmRow* rx = rows;
			const TmRow* ry = rows + dw;
			for (uint32_t idx = tid; idx < h * TM_TILE; idx += TM_BLOCK) {
				const uint32_t r = idx / TM_TILE, c = idx % TM_TILE;
				if (c >= dw) continue;
				const uint32_t n0 = rx[c].n0, n = rx[c].n < TM_MAX_TAPS ? rx[c].n : TM_MAX_TAPS;
				TmPx acc = tm_zero();
				if (n0 + n <= w) // (always: the taps lie inside the row)
					for (uint32_t k = 0; k < n; ++k) acc = tm_tap(acc, rx[c].c[k], tm_decode(src[r * w + n0 + k], decode));
				s_h[0][r][c] = acc.r;
				s_h[1][r][c] = acc.g;
				s_h[2][r][c] = acc.b;
				s_h[3][r][c] = acc.a;
				s_h[4][r][c] = acc.ra;
				s_h[5][r][c] = acc.ga;
				s_h[6][r][c] = acc.ba;
			}
			__syncthreads();
			if (mine) {
				const uint32_t n0 = ry[oy].n0, n = ry[oy].n < TM_MAX_TAPS ? ry[oy].n : TM_MAX_TAPS;
				TmPx acc = tm_zero();
				if (n0 + n <= h)
					for (uint32_t k = 0; k < n; ++k) {
						const uint32_t r = n0 + k;
						acc = tm_tap(acc, ry[oy].c[k], TmPx{s_h[0][r][ox], s_h[1][r][ox], s_h[2][r][ox], s_h[3][r][ox], s_h[4][r][ox], s_h[5][r][ox], s_h[6][r][ox]});
					}
				px = tm_encode(acc, encode);
			}
		}
		if (T.count) { // (block-uniform) scaleCoverage: the level made is what the next is made from
			if (mine) atomicAdd(&s_hist[px >> 24], 1u);
			__syncthreads();
			const float scale = tm_coverage_scale(s_hist, dw * dh, T.ref_norm, wanted);
			if (mine) px = tm_scale_alpha(px, scale);
		}
		at += w * h;
		if (mine) {
			s_px[cur ^ 1u][oy * dw + ox] = px;
			chain[at + oy * dw + ox] = px;
		}
		if (MODE != TM_STOCHASTIC) rows += dw + dh;
		w = dw;
		h = dh;
		cur ^= 1u;
		__syncthreads(); // the bins and the planes are free again
	}
}

__global__ __launch_bounds__(TM_BLOCK) void k_mip_scale(uint32_t* __restrict__ chains, uint32_t chain_px, uint32_t at, uint32_t pixels, const uint32_t* __restrict__ histogram,
	const uint32_t* __restrict__ count, uint32_t count_pixels, float ref_norm) {
	__shared__ uint32_t s_hist[256];
	const uint32_t tid = threadIdx.x, img = blockIdx.y;
	s_hist[tid] = histogram[(size_t)img * 256 + tid];
	__syncthreads();
	const float scale = tm_coverage_scale(s_hist, pixels, ref_norm, tm_coverage(*count, count_pixels));
	uint32_t* level = chains + (size_t)img * chain_px + at;
#pragma unroll
	for (uint32_t q = 0; q < TM_SCALE_PER_THREAD; ++q) {
		const uint32_t idx = (blockIdx.x * TM_SCALE_PER_THREAD + q) * TM_BLOCK + tid;
		if (idx < pixels) level[idx] = tm_scale_alpha(level[idx], scale);
	}
}

__global__ __launch_bounds__(TM_BLOCK) void k_mip_coverage(const uint32_t* __restrict__ rgba, uint32_t pixels, uint32_t ref, uint32_t* __restrict__ count) {
	__shared__ uint32_t s_count;
	if (threadIdx.x == 0) s_count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t idx = blockIdx.x * TM_BLOCK + threadIdx.x; idx < pixels; idx += gridDim.x * TM_BLOCK) mine += (rgba[idx] >> 24) > ref ? 1u : 0u;
	if (mine) atomicAdd(&s_count, mine);
	__syncthreads();
	if (threadIdx.x == 0 && s_count) atomicAdd(count, s_count);
}

} // namespace

hipError_t launch_mip_level(hipStream_t s, int mode, const TmLevel& L, uint32_t window_x, uint32_t window_y) {
	if (!L.chains || L.n_images == 0 || L.n_images > 65535u || L.w == 0 || L.h == 0 || L.dst_w == 0 || L.dst_h == 0 || L.dst_w > L.w || L.dst_h > L.h) return hipErrorInvalidValue;
	if ((uint64_t)L.src_at + (uint64_t)L.w * L.h > L.chain_px || (uint64_t)L.dst_at + (uint64_t)L.dst_w * L.dst_h > L.chain_px) return hipErrorInvalidValue;
	if (mode == TM_STOCHASTIC) {
		if (L.w > TM_STOCHASTIC_MAX_SIDE || L.h > TM_STOCHASTIC_MAX_SIDE) return hipErrorInvalidValue;
		const uint32_t grid = (L.dst_w * L.dst_h + TM_BLOCK - 1) / TM_BLOCK;
		hipLaunchKernelGGL(k_mip_level<TM_STOCHASTIC>, dim3(grid, L.n_images), dim3(TM_BLOCK), 0, s, L);
		return hipGetLastError();
	}
	if ((mode != TM_LINEAR && mode != TM_SRGB) || !L.rows_x || !L.rows_y || !L.tables || window_x > TM_WINDOW || window_y > TM_WINDOW) return hipErrorInvalidValue;
	const uint32_t grid = ((L.dst_w + TM_TILE - 1) / TM_TILE) * ((L.dst_h + TM_TILE - 1) / TM_TILE);
	if (mode == TM_SRGB) hipLaunchKernelGGL(k_mip_level<TM_SRGB>, dim3(grid, L.n_images), dim3(TM_BLOCK), 0, s, L);
	else hipLaunchKernelGGL(k_mip_level<TM_LINEAR>, dim3(grid, L.n_images), dim3(TM_BLOCK), 0, s, L);
	return hipGetLastError();
}

hipError_t launch_mip_tail(hipStream_t s, int mode, const TmTail& T) {
	if (!T.chains || T.n_images == 0 || T.w == 0 || T.h == 0 || T.w > TM_TAIL_SIDE || T.h > TM_TAIL_SIDE || (T.count && T.count_pixels == 0)) return hipErrorInvalidValue;
	if ((uint64_t)T.at + tm_chain_pixels(T.w, T.h) > T.chain_px) return hipErrorInvalidValue; // the levels behind a level are the chain of an image of its size
	if (T.w == 1 && T.h == 1) return hipSuccess;                                                // (no level to make)
	if (mode == TM_STOCHASTIC) hipLaunchKernelGGL(k_mip_tail<TM_STOCHASTIC>, dim3(T.n_images), dim3(TM_BLOCK), 0, s, T);
	else if (!T.rows || !T.tables) return hipErrorInvalidValue;
	else if (mode == TM_SRGB) hipLaunchKernelGGL(k_mip_tail<TM_SRGB>, dim3(T.n_images), dim3(TM_BLOCK), 0, s, T);
	else if (mode == TM_LINEAR) hipLaunchKernelGGL(k_mip_tail<TM_LINEAR>, dim3(T.n_images), dim3(TM_BLOCK), 0, s, T);
	else return hipErrorInvalidValue;
	return hipGetLastError();
}

hipError_t launch_mip_coverage(hipStream_t s, const uint32_t* rgba, uint32_t pixels, uint32_t ref, uint32_t* count) {
	if (!rgba || !count || pixels == 0 || ref > 255u) return hipErrorInvalidValue;
	const uint32_t want = (pixels + TM_BLOCK - 1) / TM_BLOCK;
	hipLaunchKernelGGL(k_mip_coverage, dim3(want < 1024u ? want : 1024u), dim3(TM_BLOCK), 0, s, rgba, pixels, ref, count);
	return hipGetLastError();
}

hipError_t launch_mip_scale(hipStream_t s, uint32_t* chains, uint32_t n_images, uint32_t chain_px, uint32_t at, uint32_t pixels, const uint32_t* histogram, const uint32_t* count,
	uint32_t count_pixels, float ref_norm) {
	if (!chains || !histogram || !count || n_images == 0 || n_images > 65535u || pixels == 0 || count_pixels == 0 || (uint64_t)at + pixels > chain_px) return hipErrorInvalidValue;
	const uint32_t per = TM_BLOCK * TM_SCALE_PER_THREAD;
	hipLaunchKernelGGL(k_mip_scale, dim3((pixels + per - 1) / per, n_images), dim3(TM_BLOCK), 0, s, chains, chain_px, at, pixels, histogram, count, count_pixels, ref_norm);
	return hipGetLastError();
}

} // namespace lmx
