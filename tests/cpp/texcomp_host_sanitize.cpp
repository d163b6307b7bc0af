// texcomp_host_sanitize.cpp — the host side of csrc/lmx_texcomp.h (the generated tables, the whole BC1 block encoder, BC4, the batch's layout
// and texel fetch) at its edges, as a stand-alone program: tests/test_texcomp_cpu.py builds it with -fsanitize=address,undefined and expects
// it to run clean. The blocks are chosen for the routes that index a table or shift by a computed amount: solid blocks of every grey level,
// extremes (the rounding leaves [0, 31] / [0, 63]), one pixel off a solid block (a determinant of 0), noise.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "lmx_texcomp.h"

using namespace lmx;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
	rng_state = rng_state * 1664525u + 1013904223u;
	return rng_state >> 8;
}

// the ideal decode of a block, for the error the encoder reports
static uint32_t decoded_error(const uint32_t px[16], TcBlock blk) {
	const uint32_t c0 = blk.w0 & 0xffffu, c1 = blk.w0 >> 16;
	int pal[4][3];
	const uint32_t c[2] = {c0, c1};
	for (int k = 0; k < 2; ++k) {
		pal[k][0] = tc_expand5((int)(c[k] >> 11));
		pal[k][1] = tc_expand6((int)((c[k] >> 5) & 63u));
		pal[k][2] = tc_expand5((int)(c[k] & 31u));
	}
	for (int ch = 0; ch < 3; ++ch) {
		pal[2][ch] = c0 > c1 ? (pal[0][ch] * 2 + pal[1][ch]) / 3 : (pal[0][ch] + pal[1][ch]) / 2;
		pal[3][ch] = c0 > c1 ? (pal[1][ch] * 2 + pal[0][ch]) / 3 : 0;
	}
	uint32_t err = 0;
	for (int i = 0; i < 16; ++i) {
		const int* p = pal[(blk.w1 >> (2 * i)) & 3u];
		err += (uint32_t)(tc_sq(p[0] - (int)tc_r(px[i])) + tc_sq(p[1] - (int)tc_g(px[i])) + tc_sq(p[2] - (int)tc_b(px[i])));
	}
	return err;
}

int main() {
	std::unique_ptr<TcTables> t(new TcTables());
	tc_build_tables(t.get());
	// the tables: every histogram at its own index, the all-16 entries, the midpoints ascending
	uint32_t n = 0, any16 = 0;
	for (uint32_t a = 0; a <= 16; ++a)
		for (uint32_t b = 0; a + b <= 16; ++b)
			for (uint32_t c = 0; a + b + c <= 16; ++c) {
				const uint8_t h[4] = {(uint8_t)a, (uint8_t)b, (uint8_t)c, (uint8_t)(16 - a - b - c)};
				CHECK(tc_hist_index(4, h) == n);
				CHECK((t->hist4[n].f & 255u) == a && ((t->hist4[n].f >> 16) & 255u) == a + b + c);
				any16 += t->hist4[n].f >> 24;
				++n;
			}
	CHECK(n == TC_HIST4 && any16 == 4);
	n = any16 = 0;
	for (uint32_t a = 0; a <= 16; ++a)
		for (uint32_t b = 0; a + b <= 16; ++b) {
			const uint8_t h[3] = {(uint8_t)a, (uint8_t)b, (uint8_t)(16 - a - b)};
			CHECK(tc_hist_index(3, h) == n);
			any16 += t->hist3[n].f >> 24;
			++n;
		}
	CHECK(n == TC_HIST3 && any16 == 3);
	for (int i = 0; i + 1 < 31; ++i) CHECK(t->mid5[i] < t->mid5[i + 1]);
	for (int i = 0; i + 1 < 63; ++i) CHECK(t->mid6[i] < t->mid6[i + 1]);
	CHECK(t->mid5[15] == 0.5f && t->mid6[31] == 0.5f && t->mid5[31] == 1e+37f && t->mid6[63] == 1e+37f);
	for (int k = 0; k < 4; ++k)
		for (int i = 0; i < 256; ++i) CHECK(tc_match_hi(t->match[k][i]) < (k & 1 ? 64u : 32u) && tc_match_lo(t->match[k][i]) < (k & 1 ? 64u : 32u) && tc_match_e(t->match[k][i]) < 256u);

	// blocks
	std::vector<std::vector<uint32_t>> blocks;
	for (uint32_t v = 0; v < 256; ++v) blocks.push_back(std::vector<uint32_t>(16, v * 0x010101u | 0xff000000u)); // solid greys
	for (int k = 0; k < 64; ++k) {
		std::vector<uint32_t> noise(16), ext(16), off(16, rnd() | 0xff000000u), two(16);
		const uint32_t a = rnd(), b = rnd();
		for (int i = 0; i < 16; ++i) {
			noise[i] = rnd() | rnd() << 24;
			ext[i] = (rnd() & 1 ? 0xffu : 0u) | (rnd() & 1 ? 0xff00u : 0u) | (rnd() & 1 ? 0xff0000u : 0u);
			if ((rnd() & 3) == 0) ext[i] = rnd();
			two[i] = rnd() & 1 ? a : b;
		}
		off[rnd() & 15] ^= 1u << (8 * (rnd() % 3));
		blocks.push_back(noise);
		blocks.push_back(ext);
		blocks.push_back(off);
		blocks.push_back(two);
	}
	for (const auto& px : blocks)
		for (int allow3 = 0; allow3 < 2; ++allow3) {
			uint32_t err = 0;
			const TcBlock blk = tc_encode_bc1_host(px.data(), allow3 != 0, *t, &err);
			if (!allow3) CHECK((blk.w0 & 0xffffu) > (blk.w0 >> 16));
			if (!tc_solid(px.data())) CHECK(decoded_error(px.data(), blk) == err);
			for (uint32_t shift = 0; shift <= 24; shift += 8) {
				const TcBlock a = tc_encode_bc4(px.data(), shift);
				CHECK((a.w0 & 255u) >= ((a.w0 >> 8) & 255u));
			}
		}

	// the batch: every block of every image lies in its image, texels outside are 0
	const uint32_t sizes[][2] = {{1, 1}, {2, 2}, {6, 2}, {4, 8}, {13, 9}, {4, 4}};
	std::vector<TcImage> images;
	std::vector<uint32_t> rgba;
	uint32_t n_blocks = 0;
	for (const auto& s : sizes) {
		images.push_back(TcImage{s[0], s[1], (uint32_t)rgba.size(), n_blocks});
		for (uint32_t i = 0; i < s[0] * s[1]; ++i) rgba.push_back(rnd() | 0x01000000u); // (never 0)
		n_blocks += tc_blocks_of(s[0], s[1]);
	}
	uint64_t inside = 0;
	for (uint32_t b = 0; b < n_blocks; ++b) {
		const uint32_t k = tc_image_of(images.data(), (uint32_t)images.size(), b);
		CHECK(images[k].block_at <= b && b < images[k].block_at + tc_blocks_of(images[k].w, images[k].h));
		for (uint32_t i = 0; i < 16; ++i) inside += tc_texel(images[k], rgba.data(), b, i) != 0;
	}
	CHECK(inside == rgba.size());

	if (failures) return 1;
	printf("clean: %zu blocks\n", blocks.size());
	return 0;
}
