// probes_host_sanitize.cpp — the host-side arithmetic of csrc/lmx_probes.h (the sample table, the batch and layout arithmetic, the cube
// sampler, one filter sample, the RGBM encoding, the SH table's functions) at its edges, as a stand-alone program:
// tests/test_probes_cpu.py builds it with -fsanitize=address,undefined and expects it to run clean. Inputs are what the C ABI lets
// through and what it refuses on the way in.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "lmx_probes.h"

using namespace lmx;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const float edge[] = {0.f, -0.f, 0.5f, -0.3f, 1.f, -1.f, 0.999f, 1.0000001f, 2147483520.f, 2147483648.f, -2147483904.f, 3e38f, -3e38f, inf, -inf, nan, FLT_MIN, -FLT_MIN, 1e-45f};
	// the batch's bytes and the layouts: every n and size has a defined answer inside 64 bits
	const uint32_t counts[] = {0u, 1u, 2u, 16u, 128u, 682u, 683u, 4096u, 4097u, 65535u, 65536u, 0x7fffffffu, 0xffffffffu};
	for (uint32_t n : counts)
		for (uint32_t S : counts) {
			const uint64_t bytes = probe_batch_bytes(n, S);
			CHECK(bytes <= PROBES_MAX_BATCH_BYTES);
			if (bytes) CHECK(bytes == 96ull * S * S * n && probe_texels(S) == 6ull * S * S);
		}
	CHECK(probe_batch_bytes(682, 128) != 0 && probe_batch_bytes(683, 128) == 0 && probe_batch_bytes(1, 4096) == 0 && probe_batch_bytes(1, 2048) != 0);
	for (uint32_t S : {16u, 32u, 128u, 4096u}) {
		const uint32_t last = probe_log2(S);
		CHECK((1u << last) == S && probe_is_pow2(S) && !probe_is_pow2(S + 1) && !probe_is_pow2(0));
		CHECK(probe_mip_offset(S, 1) == 0 && probe_mip_offset(S, 2) == 6ull * (S / 2) * (S / 2));
		CHECK(probe_mip_offset(S, last + 1) == 2ull * S * S - 2); // 6 (S^2 / 4 + ... + 1)
		CHECK(probe_level_offset(S, 0) == 0 && probe_level_offset(S, 1) == 6ull * S * S);
		uint64_t at = 0; // the RGBM images tile a cubemap's bytes: per face, levels 0 .. 4
		for (uint32_t face = 0; face < 6; ++face)
			for (uint32_t level = 0; level < GGX_LEVELS; ++level) {
				CHECK(probe_rgbm_offset(S, face, level) == at);
				at += (uint64_t)(S >> level) * (S >> level);
			}
		CHECK(at == probe_level_offset(S, GGX_LEVELS));
	}
	// the sample table: unit vectors, the pole at roughness 0, every level finite
	for (uint32_t level = 0; level < GGX_LEVELS; ++level)
		for (uint32_t i = 0; i < GGX_SAMPLES; ++i) {
			const V3 h = ggx_sample_h(i, (float)level / 4.f);
			CHECK(std::isfinite(h.x) && std::isfinite(h.y) && std::isfinite(h.z) && h.z >= 0.f && h.z <= 1.f);
			CHECK(std::fabs(std::sqrt((double)h.x * h.x + (double)h.y * h.y + (double)h.z * h.z) - 1.0) < 1e-6);
			if (level == 0) CHECK(h.x == 0.f && h.y == 0.f && h.z == 1.f);
		}
	CHECK(ggx_radical_inverse(0) == 0.f && ggx_radical_inverse(1) == 0.5f && ggx_radical_inverse(0xffffffffu) <= 1.f);
	// the sampler: any direction and lod, finite or not, reads inside the chain
	const uint32_t S = 16, last = 4;
	std::vector<std::vector<float>> chain(last + 1);
	for (uint32_t m = 0; m <= last; ++m) chain[m].assign(6 * (S >> m) * (S >> m) * 3, (float)m + 0.25f);
	uint64_t fetched = 0;
	auto fetch = [&](uint32_t mip, uint32_t face, uint32_t x, uint32_t y) {
		const uint32_t s = S >> mip;
		const bool ok = mip <= last && face < 6 && x < s && y < s;
		CHECK(ok);
		++fetched;
		if (!ok) return V3{0, 0, 0};
		const float* t = chain[mip].data() + 3 * ((face * s + y) * s + x);
		return V3{t[0], t[1], t[2]};
	};
	for (float x : edge)
		for (float y : edge)
			for (float z : {0.f, 1.f, -1.f, 3e38f, nan})
				for (float lod : {0.f, 0.5f, 3.999f, 4.f, 4.5f, 1e30f, -1.f, -inf, inf, nan}) (void)cube_sample(V3{x, y, z}, lod, last, fetch);
	CHECK(fetched > 0);
	for (uint32_t face = 0; face < 6; ++face) // a texel's own direction falls into that texel, whatever the mip
		for (uint32_t s : {1u, 2u, 16u, 4096u})
			for (uint32_t x : {0u, s / 2, s - 1})
				for (uint32_t y : {0u, s / 3, s - 1}) {
					const CubeCoord c = cube_dir_coord(probe_texel_dir(x, y, face, s));
					CHECK(c.face == face && cube_floor((c.a + 1.f) * 0.5f * (float)s) == (int32_t)x && cube_floor((c.b + 1.f) * 0.5f * (float)s) == (int32_t)y);
				}
	CHECK(cube_floor(-0.5f) == -1 && cube_floor(-1.f) == -1 && cube_floor(2.9f) == 2 && cube_floor(nan) == 0 && cube_floor(3e38f) == 0);
	const V3 centre = cube_sample(V3{0, 0, 5}, 1.5f, last, fetch);
	CHECK(centre.x == 1.75f);
	// one filter sample for normals on the axes and edges, the frame's switch at |N.z| = 0.999 included
	for (V3 n : {V3{0, 0, 1}, V3{0, 0, -1}, V3{1, 0, 0}, V3{0.0447f, 0, 0.999f}, V3{0.6f, 0.8f, 0}, V3{0.57735f, 0.57735f, 0.57735f}})
		for (uint32_t level = 1; level < GGX_LEVELS; ++level)
			for (uint32_t i = 0; i < GGX_SAMPLES; ++i) {
				const GgxSample q = ggx_sample(n, ggx_sample_h(i, (float)level / 4.f), (float)level / 4.f);
				const float lod = ggx_lod_clamp(log2f(q.lod_argument));
				CHECK(lod >= 0.f && lod <= 4.f);
				if (q.ndotl > 0.f) (void)cube_sample(q.L, lod, last, fetch);
			}
	CHECK(ggx_lod_clamp(nan) == 0.f && ggx_lod_clamp(-inf) == 0.f && ggx_lod_clamp(inf) == 4.f);
	// RGBM of any three floats
	for (float x : edge)
		for (float y : edge)
			for (float z : edge) {
				uint8_t q[4];
				rgbm_encode(x, y, z, q);
				CHECK(q[3] >= 1);
			}
	uint8_t q[4];
	rgbm_encode(1.f, 0.5f, -2.f, q);
	CHECK(q[0] == 255 && q[1] == 128 && q[2] == 0 && q[3] == 64);
	rgbm_encode(100.f, 4.f, 0.f, q);
	CHECK(q[0] == 255 && q[1] == 255 && q[2] == 0 && q[3] == 255);
	rgbm_encode(0.f, 0.f, 0.f, q);
	CHECK(q[0] == 0 && q[3] == 1);
	// the SH table's functions for every size the entry point lets through at its ends
	for (uint32_t w : {1u, 2u, 5u, 4096u})
		for (uint32_t face = 0; face < 6; ++face)
			for (uint32_t x : {0u, w - 1})
				for (uint32_t y : {0u, w / 2}) {
					float b[SH_COEFS];
					sh_project(sh_cube2dir(x, y, face, w), b);
					const float wt = sh_weight(x, y, w);
					CHECK(wt > 0.f && wt <= 4.f && b[0] == 0.282095f && std::isfinite(b[8]));
				}
	CHECK(sh_mult(0) == 0.282095f && sh_mult(8) == 0.546274f / 4.f && std::isfinite(sh_finish(1.f, 3.f, 4)));
	printf(failures ? "probes host arithmetic: %d checks failed\n" : "probes host arithmetic: clean\n", failures);
	return failures ? 1 : 0;
}
