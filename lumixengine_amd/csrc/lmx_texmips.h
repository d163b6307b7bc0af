// lmx_texmips.h — the arithmetic of a texture's mip chain (TextureCompressor::compress with generate_mipmaps, renderer/editor/
// render_plugins.cpp:165-215, :324-401), shared by texmips_kernels.hip and the host side of lmx_capi_texcomp.hip: the coefficient builder of
// the filtered modes, decode / encode, the seven-channel tap, the stochastic pick (downsampleNormal) and the coverage walk (computeCoverage,
// scaleCoverage). The stochastic pick and the coverage walk are the reference's, bit for bit. The filtered modes are a resampler defined
// HERE: stb_image_resize2's filter (Mitchell, stretched for downsampling, edge clamp, non-premultiplied alpha weighting),
// this file's order of the sums - horizontal pass first, each sum left to right in ascending source index, plain multiplies and adds.
// FMA-free fp32 (-ffp-contract=off); nothing here may be reassociated. The launchers are at the end.
#pragma once

#include <math.h>

#include "lmx_math.h"
#include "lmx_voxels.h" // the generator of core/math.cpp:1337-1378 and the closed form that enters its stream anywhere

namespace lmx {

constexpr int TM_LINEAR = 0, TM_SRGB = 1, TM_STOCHASTIC = 2; // LMX_TEXMIP_*
constexpr uint32_t TM_MAX_TAPS = 14;                         // 13 occur (3 -> 1); an exact 2 : 1 has 8
constexpr uint32_t TM_MAX_SIDE = 1u << 24;                   // of a chain: every texel centre p + 0.5f is exact in fp32 up to here
constexpr uint32_t TM_STOCHASTIC_MAX_SIDE = 4096;           // above, downsampleNormal's largest draw can read past a row (4163 is the first such size)

// one output texel's taps along one axis: source texels n0 .. n0 + n - 1, coefficients normalised to sum 1
struct TmRow {
	uint32_t n0, n;
	float c[TM_MAX_TAPS];
};
// generated at creation: decode[i] = the linear value of sRGB byte i; encode[k], k = 1 .. 255 = the least linear value that encodes to k
struct TmTables {
	float decode[256], encode[256];
};

LMX_HD uint32_t tm_levels(uint32_t w, uint32_t h) { // 1 + log2(max(w, h)), the integer log
	uint32_t m = w > h ? w : h, n = 0;
	while (m) {
		++n;
		m >>= 1;
	}
	return n;
}
LMX_HD uint32_t tm_side(uint32_t s, uint32_t level) { return (s >> level) ? (s >> level) : 1u; }
// the first level whose sides are both at most `side`: the levels behind it are the tail's (the last level, 1 x 1, always qualifies)
LMX_HD uint32_t tm_tail_level(uint32_t w, uint32_t h, uint32_t side) {
	uint32_t m = 0;
	while (tm_side(w, m) > side || tm_side(h, m) > side) ++m;
	return m;
}
LMX_HD uint64_t tm_chain_pixels(uint32_t w, uint32_t h) {
	uint64_t px = 0;
	const uint32_t levels = tm_levels(w, h);
	for (uint32_t m = 0; m < levels; ++m) px += (uint64_t)tm_side(w, m) * tm_side(h, m);
	return px;
}

// ---- the tables (host) --------------------------------------------------------------------------------------------------------------------
inline double tm_srgb_to_linear64(double c) { return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4); }
inline void tm_build_tables(TmTables* t) {
	for (int i = 0; i < 256; ++i) {
		// the fp32 value of the formula, rounded to six decimals. The power is powf's: the fp32 base to the fp32 exponent 2.4f, taken in fp64 and
		// rounded to fp32, so that no libm's powf decides a digit (this reproduces all 256 of stb's literals; the fp64 formula misses 11)
		const float c = (float)i / 255.0f;
		const float v = c <= 0.04045f ? c / 12.92f : (float)pow((double)((c + 0.055f) / 1.055f), (double)2.4f);
		t->decode[i] = (float)(floor((double)v * 1e6 + 0.5) / 1e6);
	}
	t->encode[0] = 0.0f; // (never read)
	for (int k = 1; k < 256; ++k) t->encode[k] = (float)tm_srgb_to_linear64(((double)k - 0.5) / 255.0);
}

// stbir__filter_mitchell (stb_image_resize2.h:2851-2864), the same fp32 expressions
inline float tm_mitchell(float x) {
	if (x < 0.0f) x = -x;
	if (x < 1.0f) return (16.0f + x * x * (21.0f * x - 36.0f)) / 18.0f;
	if (x < 2.0f) return (32.0f + x * (-60.0f + x * (36.0f - 7.0f * x))) / 18.0f;
	return 0.0f;
}

// The taps of one axis, `in` -> `out` texels (out <= in), rows[out]. out == in is a copy. Otherwise the gather form of a downsample
// (stbir__calculate_coefficients_for_gather_downsample, :3304-3380): every source texel p of [-margin, in + margin) gives its weight to the
// outputs its stretched support reaches, at texel clamp(p, 0, in - 1); then each output is normalised. false: more than TM_MAX_TAPS taps.
inline bool tm_build_coeffs(uint32_t in, uint32_t out, TmRow* rows) {
	if (in == 0 || out == 0 || out > in || in > TM_MAX_SIDE) return false; // (above 2^24, p + 0.5f is no longer exact)
	for (uint32_t o = 0; o < out; ++o) {
		rows[o].n0 = rows[o].n = 0;
		for (uint32_t k = 0; k < TM_MAX_TAPS; ++k) rows[o].c[k] = 0.0f;
	}
	if (out == in) {
		for (uint32_t o = 0; o < out; ++o) {
			rows[o].n0 = o;
			rows[o].n = 1;
			rows[o].c[0] = 1.0f;
		}
		return true;
	}
	const float scale = (float)out / (float)in;
	const float radius = 2.0f / scale;
	const int margin = (int)ceilf(4.0f / scale) / 2;
	for (int p = -margin; p < (int)in + margin; ++p) {
		const float pc = (float)p + 0.5f;
		int first = (int)floorf((pc - radius) * scale + 0.5f), last = (int)floorf((pc + radius) * scale - 0.5f);
		if (first < 0) first = 0;
		if (last >= (int)out) last = (int)out - 1;
		const uint32_t texel = p < 0 ? 0u : p >= (int)in ? in - 1 : (uint32_t)p;
		for (int o = first; o <= last; ++o) {
			const float weight = tm_mitchell(((float)o + 0.5f) - pc * scale) * scale;
			TmRow& r = rows[o];
			if (r.n == 0) r.n0 = texel; // (p ascends, and with it the texel: the first one an output sees is its lowest)
			const uint32_t k = texel - r.n0;
			if (k >= TM_MAX_TAPS) return false;
			r.c[k] = r.c[k] + weight;
			if (k + 1 > r.n) r.n = k + 1;
		}
	}
	for (uint32_t o = 0; o < out; ++o) {
		TmRow& r = rows[o];
		if (r.n == 0) return false;
		float sum = 0.0f;
		for (uint32_t k = 0; k < r.n; ++k) sum = sum + r.c[k];
		const float inv = 1.0f / sum;
		for (uint32_t k = 0; k < r.n; ++k) r.c[k] = r.c[k] * inv;
	}
	return true;
}

// ---- filtered modes: seven channels R G B A R.A G.A B.A -------------------------------------------------------------------------------------
struct TmPx {
	float r, g, b, a, ra, ga, ba;
};
LMX_HD TmPx tm_zero() { return TmPx{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
// `decode`: the sRGB table, null in linear mode
LMX_HD TmPx tm_decode(uint32_t px, const float* decode) {
	TmPx v;
	const uint32_t r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u, a = px >> 24;
	if (decode) {
		v.r = decode[r];
		v.g = decode[g];
		v.b = decode[b];
	} else {
		v.r = (float)r * (1.0f / 255.0f);
		v.g = (float)g * (1.0f / 255.0f);
		v.b = (float)b * (1.0f / 255.0f);
	}
	v.a = (float)a * (1.0f / 255.0f);
	v.ra = v.r * v.a;
	v.ga = v.g * v.a;
	v.ba = v.b * v.a;
	return v;
}
// acc + c * v, as a multiply and an add per channel
LMX_HD TmPx tm_tap(const TmPx& acc, float c, const TmPx& v) {
	TmPx o;
	o.r = acc.r + c * v.r;
	o.g = acc.g + c * v.g;
	o.b = acc.b + c * v.b;
	o.a = acc.a + c * v.a;
	o.ra = acc.ra + c * v.ra;
	o.ga = acc.ga + c * v.ga;
	o.ba = acc.ba + c * v.ba;
	return o;
}
LMX_HD uint32_t tm_encode_linear(float x) {
	const float v = x * 255.0f + 0.5f;
	return !(v > 0.0f) ? 0u : v > 255.0f ? 255u : (uint32_t)v; // (a NaN gives 0)
}
// the number of k in 1 .. 255 with encode[k] <= x (the table ascends); a NaN gives 0
LMX_HD uint32_t tm_encode_srgb(float x, const float* encode) {
	uint32_t lo = 0, hi = 256; // encode[lo] <= x (lo = 0: nothing known), encode[hi] > x
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (encode[mid] <= x) lo = mid;
		else hi = mid;
	}
	return lo;
}
// `encode`: the sRGB table, null in linear mode
LMX_HD uint32_t tm_encode(const TmPx& v, const float* encode) {
	float r = v.r, g = v.g, b = v.b;
	if (!(v.a < 7.52316384526264005e-37f)) { // 2^-120, stbir__small_float
		const float inv = 1.0f / v.a;
		r = v.ra * inv;
		g = v.ga * inv;
		b = v.ba * inv;
	}
	const uint32_t a8 = tm_encode_linear(v.a);
	if (encode) return tm_encode_srgb(r, encode) | tm_encode_srgb(g, encode) << 8 | tm_encode_srgb(b, encode) << 16 | a8 << 24;
	return tm_encode_linear(r) | tm_encode_linear(g) << 8 | tm_encode_linear(b) << 16 | a8 << 24;
}

// ---- stochastic mode: downsampleNormal (:165-200) ------------------------------------------------------------------------------------------
// the index of the source texel destination texel (i, j) copies. Row j's generator is seeded (521288629, 362436069 + 1337 j) and pixel i takes
// draws 2 i (the row's) and 2 i + 1 (the column's). For sides up to TM_STOCHASTIC_MAX_SIDE the index lies inside the image
// (tests/test_texmips_cpu.py enumerates it), so the min below never binds: it only keeps a wrong caller from reading outside the level.
LMX_HD uint32_t tm_stochastic_pick(uint32_t w, uint32_t h, uint32_t dst_w, uint32_t dst_h, uint32_t i, uint32_t j) {
	const float rw = (float)w / (float)dst_w, rh = (float)h / (float)dst_h;
	VoxelRng rg = voxel_rng_skip(VoxelRng{521288629u, 362436069u + 1337u * j}, 2ull * i);
	float r = (float)((double)rh * ((double)rg.rand() * 2.328306435996595e-10));
	float s = (float)(int32_t)j * rh;
	float r0 = 1 - (s - (float)(uint32_t)s);
	const uint32_t row = (r > r0 ? 1u : 0u) + (r > (r0 + 1) ? 1u : 0u);
	r = (float)((double)rw * ((double)rg.rand() * 2.328306435996595e-10));
	s = (float)i * rw;
	r0 = 1 - (s - (float)(uint32_t)s);
	const uint32_t col = (r > r0 ? 1u : 0u) + (r > (r0 + 1) ? 1u : 0u);
	const uint32_t isrc = (uint32_t)((float)i * rw) + col, jsrc = (uint32_t)((float)(int32_t)j * rh) + row;
	const uint32_t at = isrc + jsrc * w, last = w * h - 1u;
	return at < last ? at : last;
}

// ---- coverage: computeCoverage / scaleCoverage (:324-357) ---------------------------------------------------------------------------------
LMX_HD uint32_t tm_u8_clamped(float v) { return !(v > 0.0f) ? 0u : v > 255.0f ? 255u : (uint32_t)v; } // u8(clamp(v, 0, 255)); a NaN gives 0
LMX_HD uint32_t tm_coverage_ref(float ref_norm) { return tm_u8_clamped(255 * ref_norm); }
LMX_HD float tm_coverage(uint32_t count, uint32_t pixels) { return (float)((double)count / (double)pixels); }
// the factor scaleCoverage gives a level's alpha, from its 256-bin alpha histogram; may be infinite (new_ref == 0) or NaN (ref_norm == 0 too)
LMX_HD float tm_coverage_scale(const uint32_t* histogram, uint32_t pixels, float ref_norm, float coverage) {
	uint32_t count = (uint32_t)((float)pixels * (1 - coverage));
	float new_ref;
	for (new_ref = 0; new_ref < 255; ++new_ref) {
		const uint32_t bin = histogram[(uint32_t)new_ref];
		if (count < bin) {
			new_ref += (float)count / (float)bin;
			break;
		}
		count -= bin;
	}
	return ref_norm / (new_ref / 255.f);
}
LMX_HD uint32_t tm_scale_alpha(uint32_t px, float scale) { return (px & 0xffffffu) | tm_u8_clamped((float)(px >> 24) * scale) << 24; }

// ---- a whole level on the host: what k_mip_level computes, sequentially (the CPU tests and the sanitizer program run this) --------------------
// scratch: src_h x dst_w TmPx for the filtered modes (unused in stochastic mode)
inline void tm_level_host(int mode, const uint32_t* src, uint32_t w, uint32_t h, uint32_t* dst, uint32_t dst_w, uint32_t dst_h, const TmRow* rows_x, const TmRow* rows_y, const TmTables& t,
	TmPx* scratch) {
	if (mode == TM_STOCHASTIC) {
		for (uint32_t j = 0; j < dst_h; ++j)
			for (uint32_t i = 0; i < dst_w; ++i) dst[i + j * dst_w] = src[tm_stochastic_pick(w, h, dst_w, dst_h, i, j)];
		return;
	}
	const float* decode = mode == TM_SRGB ? t.decode : nullptr;
	const float* encode = mode == TM_SRGB ? t.encode : nullptr;
	for (uint32_t y = 0; y < h; ++y)
		for (uint32_t ox = 0; ox < dst_w; ++ox) {
			const TmRow& r = rows_x[ox];
			TmPx acc = tm_zero();
			for (uint32_t k = 0; k < r.n; ++k) acc = tm_tap(acc, r.c[k], tm_decode(src[y * w + r.n0 + k], decode));
			scratch[(size_t)y * dst_w + ox] = acc;
		}
	for (uint32_t oy = 0; oy < dst_h; ++oy)
		for (uint32_t ox = 0; ox < dst_w; ++ox) {
			const TmRow& r = rows_y[oy];
			TmPx acc = tm_zero();
			for (uint32_t k = 0; k < r.n; ++k) acc = tm_tap(acc, r.c[k], scratch[(size_t)(r.n0 + k) * dst_w + ox]);
			dst[oy * dst_w + ox] = tm_encode(acc, encode);
		}
}

#if defined(__HIPCC__)
// ---- texmips_kernels.hip ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t TM_BLOCK = 256; // threads of a workgroup
constexpr uint32_t TM_TILE = 16;   // a workgroup of k_mip_level makes TM_TILE x TM_TILE output texels
constexpr uint32_t TM_WINDOW = 48; // source texels per axis a tile may need: 15 x (2 + 1 / 16) + 10 taps at most for a full tile, 13 for the 3 -> 1 of a tile of one
constexpr uint32_t TM_SCALE_PER_THREAD = 4; // texels a lane of k_mip_scale rescales
constexpr uint32_t TM_TAIL_SIDE = 32;       // once both sides of a level are at most this, k_mip_tail makes all levels behind it

// every image of the batch is a chain of `chain_px` texels behind `chains`; the level read lies `src_at` texels into it, the level written `dst_at`
struct TmLevel {
	uint32_t* chains;
	uint32_t n_images, chain_px, src_at, dst_at;
	uint32_t w, h, dst_w, dst_h;
	const TmRow* rows_x; // dst_w rows, then (rows_y) dst_h rows; unused in stochastic mode
	const TmRow* rows_y;
	const TmTables* tables;
	uint32_t* histogram; // n_images x 256 bins of the written level's alpha, zero before the launch; null: not gathered
};
// largest source window any tile of this level needs along an axis (host): the launch is refused above TM_WINDOW
inline uint32_t tm_max_window(const TmRow* rows, uint32_t out) {
	uint32_t worst = 0;
	for (uint32_t o0 = 0; o0 < out; o0 += TM_TILE) {
		const uint32_t o1 = o0 + TM_TILE < out ? o0 + TM_TILE - 1 : out - 1;
		uint32_t hi = rows[o0].n0 + rows[o0].n;
		for (uint32_t o = o0; o <= o1; ++o) {
			if (rows[o].n0 < rows[o0].n0) return 0xffffffffu; // (the first texel of a tile's first output is the tile's lowest)
			hi = rows[o].n0 + rows[o].n > hi ? rows[o].n0 + rows[o].n : hi;
		}
		worst = hi - rows[o0].n0 > worst ? hi - rows[o0].n0 : worst;
	}
	return worst;
}
hipError_t launch_mip_level(hipStream_t s, int mode, const TmLevel& level, uint32_t window_x, uint32_t window_y);
// every level behind the one at `at` (w x h, both sides <= TM_TAIL_SIDE) of every chain, one workgroup per chain
struct TmTail {
	uint32_t* chains;
	uint32_t n_images, chain_px, at;
	uint32_t w, h;
	const TmRow* rows; // of the first level made: its columns' taps, its rows'; then the next level's, and so on
	const TmTables* tables;
	const uint32_t* count; // computeCoverage's count over count_pixels texels; null: no coverage scaling
	uint32_t count_pixels;
	float ref_norm;
};
hipError_t launch_mip_tail(hipStream_t s, int mode, const TmTail& tail);
// alpha > ref over `pixels` texels at `rgba`, added to *count (zero before the launch)
hipError_t launch_mip_coverage(hipStream_t s, const uint32_t* rgba, uint32_t pixels, uint32_t ref, uint32_t* count);
// scaleCoverage of the level at `at` of every chain: the factor from the level's histogram, the wanted coverage from *count over `count_pixels`
hipError_t launch_mip_scale(hipStream_t s, uint32_t* chains, uint32_t n_images, uint32_t chain_px, uint32_t at, uint32_t pixels, const uint32_t* histogram, const uint32_t* count,
	uint32_t count_pixels, float ref_norm);
#endif

} // namespace lmx
