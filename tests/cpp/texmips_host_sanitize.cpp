// texmips_host_sanitize.cpp — the host side of csrc/lmx_texmips.h (the generated tables, the coefficient builder, whole levels in the three
// modes, the coverage walk) at its edges, as a stand-alone program: tests/test_texmips_cpu.py builds it with -fsanitize=address,undefined and
// expects it to run clean. The sizes are chosen for what indexes an array by a computed amount: taps folded onto the first and last texel,
// a copied axis, 3 -> 1, the largest stochastic side, a walk that ends at 255, an infinite and a NaN factor.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lmx_texmips.h"

using namespace lmx;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
	rng_state = rng_state * 1664525u + 1013904223u;
	return rng_state >> 8;
}

static void chain(int mode, uint32_t w, uint32_t h, float ref_norm, const TmTables& tables) {
	const uint32_t levels = tm_levels(w, h);
	std::vector<uint32_t> px((size_t)tm_chain_pixels(w, h));
	for (size_t i = 0; i < (size_t)w * h; ++i) px[i] = rnd() << 8 | (rnd() & 1u ? rnd() & 255u : 0u) << 24 | (rnd() & 255u);
	std::vector<TmPx> scratch((size_t)h * tm_side(w, 1));
	uint32_t count = 0;
	for (size_t i = 0; i < (size_t)w * h; ++i) count += (px[i] >> 24) > tm_coverage_ref(ref_norm) ? 1u : 0u;
	const float wanted = tm_coverage(count, w * h);
	size_t at = 0;
	for (uint32_t m = 1; m < levels; ++m) {
		const uint32_t sw = tm_side(w, m - 1), sh = tm_side(h, m - 1), dw = tm_side(w, m), dh = tm_side(h, m);
		std::vector<TmRow> rx(dw), ry(dh); // exactly as long as the outputs: a row written past them is reported
		CHECK(tm_build_coeffs(sw, dw, rx.data()) && tm_build_coeffs(sh, dh, ry.data()));
		for (uint32_t o = 0; o < dw; ++o) CHECK(rx[o].n >= 1 && rx[o].n <= TM_MAX_TAPS && rx[o].n0 + rx[o].n <= sw);
		for (uint32_t o = 0; o < dh; ++o) CHECK(ry[o].n >= 1 && ry[o].n <= TM_MAX_TAPS && ry[o].n0 + ry[o].n <= sh);
		std::vector<uint32_t> src(px.begin() + at, px.begin() + at + (size_t)sw * sh), dst((size_t)dw * dh); // tight copies, for the same reason
		tm_level_host(mode, src.data(), sw, sh, dst.data(), dw, dh, rx.data(), ry.data(), tables, scratch.data());
		if (ref_norm >= 0) {
			uint32_t histogram[256] = {};
			for (uint32_t p : dst) ++histogram[p >> 24];
			const float scale = tm_coverage_scale(histogram, dw * dh, ref_norm, wanted);
			for (uint32_t& p : dst) p = tm_scale_alpha(p, scale);
		}
		at += (size_t)sw * sh;
		memcpy(px.data() + at, dst.data(), 4 * dst.size());
	}
}

int main() {
	TmTables tables;
	tm_build_tables(&tables);
	for (int k = 2; k < 256; ++k) CHECK(tables.encode[k] > tables.encode[k - 1] && tables.decode[k] > tables.decode[k - 1]);
	for (int k = 0; k < 256; ++k) CHECK(tm_encode_srgb(tables.decode[k], tables.encode) == (uint32_t)k && tm_encode_linear((float)k * (1.0f / 255.0f)) == (uint32_t)k); // both round-trip
	const float nan = __builtin_nanf(""), inf = __builtin_inff();
	CHECK(tm_encode_srgb(nan, tables.encode) == 0 && tm_encode_linear(nan) == 0 && tm_encode_srgb(inf, tables.encode) == 255 && tm_encode_linear(-inf) == 0 && tm_encode_linear(inf) == 255);
	CHECK(tm_u8_clamped(nan) == 0 && tm_u8_clamped(inf) == 255 && tm_u8_clamped(-1.0f) == 0 && tm_u8_clamped(254.9f) == 254);
	CHECK(tm_levels(1, 1) == 1 && tm_levels(4096, 1) == 13 && tm_levels(4097, 3) == 13 && tm_chain_pixels(4, 4) == 21);
	std::vector<TmRow> rows(1);
	CHECK(!tm_build_coeffs(2, 4, rows.data()) && !tm_build_coeffs(0, 0, rows.data()));
	const uint32_t sizes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 3}, {5, 5}, {7, 3}, {8, 8}, {37, 21}, {33, 17}, {128, 64}, {4097, 1}, {1, 4097}};
	for (const auto& s : sizes)
		for (int mode = 0; mode < 3; ++mode)
			for (float ref_norm : {-1.0f, 0.0f, 0.5f, 1.0f})
				if (mode != TM_STOCHASTIC || (s[0] <= TM_STOCHASTIC_MAX_SIDE && s[1] <= TM_STOCHASTIC_MAX_SIDE)) chain(mode, s[0], s[1], ref_norm, tables);
	chain(TM_STOCHASTIC, 4096, 3, 0.5f, tables);
	chain(TM_STOCHASTIC, 3, 4096, -1.0f, tables);
	// the walk: an empty histogram but for the last bin (no break, new_ref ends at 255), count 0 on a filled bin 0 (new_ref 0: an infinite factor; 0 / 0 with ref 0)
	uint32_t histogram[256] = {};
	histogram[255] = 10;
	CHECK(tm_coverage_scale(histogram, 10, 0.5f, 0.0f) == 0.5f / (255.0f / 255.f));
	histogram[0] = 5;
	CHECK(tm_coverage_scale(histogram, 15, 0.5f, 1.0f) == inf);
	const float none = tm_coverage_scale(histogram, 15, 0.0f, 1.0f);
	CHECK(none != none && tm_scale_alpha(0x80112233u, none) == 0x00112233u && tm_scale_alpha(0x00112233u, inf) == 0x00112233u && tm_scale_alpha(0x01112233u, inf) == 0xff112233u);
	if (failures) return 1;
	printf("clean\n");
	return 0;
}
