// animcomp_host_sanitize.cpp — csrc/lmx_animcomp.h as host code under AddressSanitizer and UndefinedBehaviorSanitizer (built and run by
// tests/test_animcomp_cpu.py; TEST INFRASTRUCTURE). Whole clips into arrays of exactly the sizes the info names, so a byte written behind a
// stream or a table is a heap overflow: 57-bit entries at every bit offset, a frame that ends inside a byte, 196 bones, one sample, the
// rotation clamp, a zero-range channel, and every refusal (whose quotients, shifts and conversions must stay defined).
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "lmx_animcomp.h"

using namespace lmx;

static uint32_t rng_state = 12345u;
static float rnd() {
	rng_state = rng_state * 1664525u + 1013904223u;
	return (float)(rng_state >> 8) / 16777216.0f;
}

struct Result {
	LmxAnimCompInfo info;
	std::vector<LmxAnimConstTranslation> ct;
	std::vector<LmxAnimTranslationTrack> tt;
	std::vector<LmxAnimConstRotation> cr;
	std::vector<LmxAnimRotationTrack> rt;
	std::vector<uint8_t> ts, rs;
};

static Result compress(uint32_t nb, uint32_t ns, const std::vector<float>& keys, const std::vector<float>& bind, const uint8_t* has_keys, float t_error, float r_error) {
	LmxAnimCompClip d{};
	d.n_bones = nb, d.n_samples = ns, d.fps = 30.f, d.translation_error = t_error, d.rotation_error = r_error;
	d.has_keys = has_keys, d.bind_positions = bind.data();
	Result r;
	if (!ac_compress_host(d, keys.data(), &r.info, nullptr)) abort();
	r.ct.resize(r.info.n_const_translations), r.tt.resize(r.info.n_translations), r.cr.resize(r.info.n_const_rotations), r.rt.resize(r.info.n_rotations);
	r.ts.resize((size_t)r.info.translation_stream_size), r.rs.resize((size_t)r.info.rotation_stream_size);
	LmxAnimCompOutput out{};
	// exact sizes: each table in its own allocation
	out.const_translations = r.ct.data(), out.translations = r.tt.data(), out.const_rotations = r.cr.data(), out.rotations = r.rt.data();
	out.translation_stream = r.ts.data(), out.rotation_stream = r.rs.data();
	out.cap_tracks = nb, out.cap_translation_stream = r.ts.size(), out.cap_rotation_stream = r.rs.size();
	if (!r.info.status) {
		std::vector<LmxAnimConstTranslation> ct(nb);
		std::vector<LmxAnimTranslationTrack> tt(nb);
		std::vector<LmxAnimConstRotation> cr(nb);
		std::vector<LmxAnimRotationTrack> rt(nb);
		out.const_translations = ct.data(), out.translations = tt.data(), out.const_rotations = cr.data(), out.rotations = rt.data();
		LmxAnimCompInfo again;
		if (!ac_compress_host(d, keys.data(), &again, &out)) abort();
		if (memcmp(&again, &r.info, sizeof(again))) abort();
		std::copy(ct.begin(), ct.begin() + r.ct.size(), r.ct.begin());
		std::copy(tt.begin(), tt.begin() + r.tt.size(), r.tt.begin());
		std::copy(cr.begin(), cr.begin() + r.cr.size(), r.cr.begin());
		std::copy(rt.begin(), rt.begin() + r.rt.size(), r.rt.begin());
		out.cap_tracks = 0; // too small: refused, nothing written
		if (nb && (r.info.n_const_rotations || r.info.n_rotations) && ac_compress_host(d, keys.data(), &again, &out)) abort();
	}
	return r;
}

// nb bones, ns samples: translation channel c of bone b spans widths[b % n][c], rotation channels span r_width
static std::vector<float> make_keys(uint32_t nb, uint32_t ns, const float (*widths)[3], uint32_t n, float r_width) {
	std::vector<float> k((size_t)nb * ns * 7);
	for (uint32_t s = 0; s < ns; ++s)
		for (uint32_t b = 0; b < nb; ++b) {
			float* key = &k[((size_t)s * nb + b) * 7];
			for (int c = 0; c < 3; ++c) key[c] = 1.f + (s == 0 ? 0.f : s == 1 ? 1.f : rnd()) * widths[b % n][c];
			for (int c = 0; c < 4; ++c) key[3 + c] = -0.5f * r_width + (s == 0 ? 0.f : s == 1 ? 1.f : rnd()) * r_width;
		}
	return k;
}

int main() {
	const float w19 = 0.00005f * 1.5f * 524288.f, w1 = 0.00005f * 3.f, w2 = 0.00005f * 6.f;
	// 57 bits behind leads of 0, 3, 4, 5, 6 and 7 bits; 1, 3 and 35 samples: the last frame ends inside a byte
	const float leads[6][2][3] = {{{w19, w19, w19}, {w19, w19, w19}}, {{w1, w1, w1}, {w19, w19, w19}}, {{w1, w1, w2}, {w19, w19, w19}}, {{w1, w2, w2}, {w19, w19, w19}},
	                              {{w2, w2, w2}, {w19, w19, w19}}, {{w2, w2, 2 * w2}, {w19, w19, w19}}};
	for (int i = 0; i < 6; ++i)
		for (uint32_t ns : {1u, 3u, 35u}) {
			const std::vector<float> keys = make_keys(2, ns, leads[i], 2, 2.f), bind(6, 0.f);
			const Result r = compress(2, ns, keys, bind, nullptr, 1.f, 1.f);
			if (r.info.status || (ns > 1 && r.info.n_translations != 2)) return 1;
		}
	{ // 196 bones of 57 bits and the clamp (four channels of 30 bits): the largest frames there are
		const float wide[1][3] = {{w19, w19, w19}};
		const std::vector<float> keys = make_keys(196, 5, wide, 1, 2.f), bind(3 * 196, 0.f);
		std::vector<uint8_t> has(196, 1);
		has[0] = has[100] = has[195] = 0;
		const Result r = compress(196, 5, keys, bind, has.data(), 1.f, 1e-3f);
		if (r.info.status || r.info.n_translations != 193 || r.info.translations_frame_size_bits != 193 * 57 || r.info.rotations_frame_size_bits != 193 * 49) return 2;
	}
	{ // a zero-range channel in an animated track, and bones at the bind pose
		const float flat[2][3] = {{w19, 0.f, w2}, {0.f, 0.f, 0.f}};
		const std::vector<float> keys = make_keys(2, 9, flat, 2, 0.f);
		const std::vector<float> bind = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
		const Result r = compress(2, 9, keys, bind, nullptr, 1.f, 1.f);
		if (r.info.status || r.info.n_translations != 1 || r.info.n_const_translations != 0 || r.info.n_const_rotations != 2) return 3;
	}
	{ // the refusals
		const float wide[1][3] = {{w19, w19, w19}};
		const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
		std::vector<float> keys = make_keys(3, 4, wide, 1, 2.f), bind(9, 0.f);
		if (compress(3, 0, keys, bind, nullptr, 1.f, 1.f).info.status != LMX_ANIMCOMP_NO_SAMPLES) return 4;
		for (float e : {0.f, -1.f, inf, nan})
			if (compress(3, 4, keys, bind, nullptr, e, 1.f).info.status != LMX_ANIMCOMP_BAD_ERROR || compress(3, 4, keys, bind, nullptr, 1.f, e).info.status != LMX_ANIMCOMP_BAD_ERROR) return 5;
		if (compress(3, 4, keys, bind, nullptr, 1e-30f, 1.f).info.status != LMX_ANIMCOMP_QUOTIENT_RANGE) return 6; // the quotient overflows to infinity
		if (compress(3, 4, keys, bind, nullptr, 1.f, 1e-4f).info.status != LMX_ANIMCOMP_QUOTIENT_RANGE) return 7;
		if (compress(3, 4, keys, bind, nullptr, 1.f / 4096.f, 1.f).info.status != LMX_ANIMCOMP_CHANNEL_BITS) return 8; // 31 bits
		if (compress(3, 4, keys, bind, nullptr, 0.5f, 1.f).info.status != LMX_ANIMCOMP_ENTRY_BITS) return 9;          // 3 x 20 bits
		for (float v : {inf, -inf, nan, 3.0e38f}) {
			std::vector<float> bad = keys;
			bad[7 * 5 + 4] = v;
			const uint32_t want = v == 3.0e38f ? (uint32_t)LMX_ANIMCOMP_QUOTIENT_RANGE : (uint32_t)LMX_ANIMCOMP_NONFINITE_KEY;
			if (compress(3, 4, bad, bind, nullptr, 1.f, 1.f).info.status != want) return 10;
			bad = keys;
			bad[2] = v == 3.0e38f ? -3.0e38f : v; // a position: the difference to the bind position and the range overflow
			bad[7 * 3 * 3 + 2] = 3.0e38f;
			if (compress(3, 4, bad, bind, nullptr, 1.f, 1.f).info.status != want) return 11;
		}
		std::vector<float> bad_bind = bind;
		bad_bind[4] = nan;
		if (compress(3, 4, keys, bad_bind, nullptr, 1.f, 1.f).info.status != LMX_ANIMCOMP_NONFINITE_BIND) return 12;
		const uint8_t has[3] = {1, 0, 1};
		if (compress(3, 4, keys, bad_bind, has, 1.f, 1.f).info.status != LMX_ANIMCOMP_OK) return 13;
	}
	printf("clean\n");
	return 0;
}
