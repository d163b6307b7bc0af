// lmx_probes.h — the arithmetic of the probe bake (renderer/editor/render_plugins.cpp), shared by probe_kernels.hip and the host side of
// lmx_capi_probes.hip: SphericalHarmonics::compute's weight, cube2dir with its own face table, project, the term of one pixel and the final
// scaling (:476-587); the `downscale` program's 2 x 2 average (:2850-2898); the cube sampler this library defines; one sample of
// data/shaders/ibl_filter.hlsl's loop with D_GGX and the lod of prefilteredImportanceSampling; saveCubemap's RGBM encoding (:3555-3559); the
// layouts of the batch and its outputs. FMA-free fp32 in the reference's operation order (-ffp-contract=off); nothing here may be
// reassociated. The launchers of the kernels are declared at the end.
#pragma once

#include "lmx_math.h"

namespace lmx {

constexpr float PROBE_PI = 3.14159265f; // core/math.h:404
constexpr uint32_t SH_COEFS = 9;
constexpr uint32_t SH_TABLE_ROWS = 10;  // per pixel: project's nine values, then the weight

// compute's weight (:558-561). u and v lie in (0, 1) here, not in (-1, 1): kept as the reference has it.
LMX_HD float sh_weight(uint32_t x, uint32_t y, uint32_t w) {
	const float u = ((float)x + 0.5f) / (float)w;
	const float v = ((float)y + 0.5f) / (float)w;
	const float temp = (1.0f + u * u) + v * v;
	return 4.0f / (sqrtf(temp) * temp);
}

// cube2dir (:524-541) with its face table (:531-538); not the radiance filter's
LMX_HD V3 sh_cube2dir(uint32_t x, uint32_t y, uint32_t face, uint32_t w) {
	const float u = (((float)x + 0.5f) / (float)w) * 2.f - 1.f;
	float v = (((float)y + 0.5f) / (float)w) * 2.f - 1.f;
	v *= -1.f;
	switch (face) {
		case 0: return normalize(V3{1.f, v, -u});
		case 1: return normalize(V3{-1.f, v, u});
		case 2: return normalize(V3{u, 1.f, -v});
		case 3: return normalize(V3{u, -1.f, v});
		case 4: return normalize(V3{u, v, 1.f});
		case 5: return normalize(V3{-u, v, -1.f});
	}
	return V3{0.f, 0.f, 0.f};
}

// project (:507-521): the products are left-associated
LMX_HD void sh_project(V3 dir, float b[SH_COEFS]) {
	b[0] = 0.282095f;
	b[1] = 0.488603f * dir.y;
	b[2] = 0.488603f * dir.z;
	b[3] = 0.488603f * dir.x;
	b[4] = 1.092548f * dir.x * dir.y;
	b[5] = 1.092548f * dir.y * dir.z;
	b[6] = 0.315392f * (3.0f * dir.z * dir.z - 1.0f);
	b[7] = 1.092548f * dir.x * dir.z;
	b[8] = 0.546274f * (dir.x * dir.x - dir.y * dir.y);
}

// `project(dir) * (color * weight)` (:564), one coefficient and channel
LMX_HD float sh_term(float basis, float color, float weight) { return basis * (color * weight); }

// mults (:571-581): fp32 constant expressions
LMX_HD float sh_mult(uint32_t i) {
	switch (i) {
		case 0: return 0.282095f;
		case 1:
		case 2:
		case 3: return 0.488603f * 2 / 3.f;
		case 4:
		case 5:
		case 7: return 1.092548f / 4.f;
		case 6: return 0.315392f / 4.f;
	}
	return 0.546274f / 4.f;
}

// `*this = *this * ((4.0f * PI) / weightSum)` (:569), then `coefs[i] * mults[i]` (:583-585)
LMX_HD float sh_finish(float sum, float weight_sum, uint32_t i) { return (sum * ((4.0f * PROBE_PI) / weight_sum)) * sh_mult(i); }

// the `downscale` program's texel (:2850-2898): (((0 + v00) + v10) + v01) + v11 in its i-inner, j-outer order, times 0.25f
LMX_HD float mip_average(float v00, float v10, float v01, float v11) { return ((((0.f + v00) + v10) + v01) + v11) * 0.25f; }

// ---- the cube sampler (ours to define: hardware filtering is implementation-defined) --------------------------------------
// A point of a face: a and b in [-1, 1] run with the texel columns and rows (x and y of the readTexture layout).
struct CubeCoord {
	uint32_t face;
	float a, b;
};

// ibl_filter.hlsl's `switch (u_face)` (:83-90) with its uv = (a, b): the direction of a point of a face's plane, not normalized.
// a and b may lie outside [-1, 1]: the face's extended plane.
LMX_HD V3 cube_face_dir(uint32_t face, float a, float b) {
	switch (face) {
		case 0: return V3{1.f, -b, -a};
		case 1: return V3{-1.f, -b, a};
		case 2: return V3{a, 1.f, b};
		case 3: return V3{a, -1.f, -b};
		case 4: return V3{a, -b, 1.f};
	}
	return V3{-a, -b, -1.f};
}

// The direction of texel (x, y) of a face of an output level of size s, as the shader computes it: mainVS flips pos.y, so the pixel's
// in_uv is ((x + 0.5) / s, 1 - (y + 0.5) / s); mainPS takes `uv = in_uv * 2 - 1`, `uv.y *= -1`, and the table above.
LMX_HD V3 probe_texel_dir(uint32_t x, uint32_t y, uint32_t face, uint32_t s) {
	const float a = (((float)x + 0.5f) / (float)s) * 2.f - 1.f;
	float b = (1.f - ((float)y + 0.5f) / (float)s) * 2.f - 1.f;
	b *= -1.f;
	return cube_face_dir(face, a, b);
}

// direction -> face and point: the major axis picks the face (ties in x, y, z order); the inverse of cube_face_dir
LMX_HD CubeCoord cube_dir_coord(V3 d) {
	const float ax = abs_f(d.x), ay = abs_f(d.y), az = abs_f(d.z);
	CubeCoord c;
	if (ax >= ay && ax >= az) {
		c.face = d.x < 0 ? 1u : 0u;
		c.a = (d.x < 0 ? d.z : -d.z) / ax;
		c.b = -d.y / ax;
	} else if (ay >= az) {
		c.face = d.y < 0 ? 3u : 2u;
		c.a = d.x / ay;
		c.b = (d.y < 0 ? -d.z : d.z) / ay;
	} else {
		c.face = d.z < 0 ? 5u : 4u;
		c.a = (d.z < 0 ? -d.x : d.x) / az;
		c.b = -d.y / az;
	}
	return c;
}

// floor for the sampler's coordinates (|v| far below 2^31); NaN gives 0
LMX_HD int32_t cube_floor(float v) {
	if (!(v > -1.0e9f && v < 1.0e9f)) return 0;
	const int32_t i = (int32_t)v;
	return (float)i > v ? i - 1 : i;
}
LMX_HD int32_t cube_clamp_i(int32_t v, int32_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The texel (x, y) of `face` in a mip of size s, where x and y may lie one texel outside the face: such a texel's centre, on the face's
// extended plane, is taken as a direction, and the texel that direction falls into is read. `fetch(face, x, y)` reads inside a face.
template <typename Fetch> LMX_HD V3 cube_texel(uint32_t face, int32_t x, int32_t y, int32_t s, Fetch fetch) {
	if (x >= 0 && x < s && y >= 0 && y < s) return fetch(face, (uint32_t)x, (uint32_t)y);
	const float a = (((float)x + 0.5f) / (float)s) * 2.f - 1.f;
	const float b = (((float)y + 0.5f) / (float)s) * 2.f - 1.f;
	const CubeCoord c = cube_dir_coord(cube_face_dir(face, a, b));
	const int32_t xi = cube_clamp_i(cube_floor((c.a + 1.f) * 0.5f * (float)s), s - 1);
	const int32_t yi = cube_clamp_i(cube_floor((c.b + 1.f) * 0.5f * (float)s), s - 1);
	return fetch(c.face, (uint32_t)xi, (uint32_t)yi);
}

LMX_HD V3 cube_lerp(V3 p, V3 q, float t) { return V3{p.x + (q.x - p.x) * t, p.y + (q.y - p.y) * t, p.z + (q.z - p.z) * t}; } // the one lerp form

// bilinear in one mip of size s, texel centres at + 0.5
template <typename Fetch> LMX_HD V3 cube_bilinear(CubeCoord c, int32_t s, Fetch fetch) {
	const float fx = (c.a + 1.f) * 0.5f * (float)s - 0.5f;
	const float fy = (c.b + 1.f) * 0.5f * (float)s - 0.5f;
	const int32_t x0 = cube_clamp_i(cube_floor(fx) + 1, s) - 1, y0 = cube_clamp_i(cube_floor(fy) + 1, s) - 1; // in [-1, s - 1] whatever the direction was
	const float tx = fx - (float)x0, ty = fy - (float)y0;
	const V3 t00 = cube_texel(c.face, x0, y0, s, fetch), t10 = cube_texel(c.face, x0 + 1, y0, s, fetch);
	const V3 t01 = cube_texel(c.face, x0, y0 + 1, s, fetch), t11 = cube_texel(c.face, x0 + 1, y0 + 1, s, fetch);
	return cube_lerp(cube_lerp(t00, t10, tx), cube_lerp(t01, t11, tx), ty);
}

// trilinear: `lod` below 0 reads mip 0, past the last mip the last one. `fetch(mip, face, x, y)` reads a texel of the chain of a cubemap
// of size S = 1 << last_mip.
template <typename Fetch> LMX_HD V3 cube_sample(V3 dir, float lod, uint32_t last_mip, Fetch fetch) {
	const CubeCoord c = cube_dir_coord(dir);
	const float top = (float)last_mip;
	const float l = lod > 0.f ? (lod < top ? lod : top) : 0.f; // (NaN reads mip 0)
	const uint32_t m0 = (uint32_t)cube_floor(l);
	const uint32_t m1 = m0 < last_mip ? m0 + 1 : last_mip;
	const float t = l - (float)m0;
	const V3 c0 = cube_bilinear(c, (int32_t)(1u << (last_mip - m0)), [&](uint32_t face, uint32_t x, uint32_t y) { return fetch(m0, face, x, y); });
	const V3 c1 = cube_bilinear(c, (int32_t)(1u << (last_mip - m1)), [&](uint32_t face, uint32_t x, uint32_t y) { return fetch(m1, face, x, y); });
	return cube_lerp(c0, c1, t);
}

// ---- the radiance filter (data/shaders/ibl_filter.hlsl, mainPS) -----------------------------------------------------------------------------
constexpr uint32_t GGX_SAMPLES = 128; // SAMPLE_COUNT
constexpr uint32_t GGX_LEVELS = 5;    // roughness_levels (:3704): roughness = level / 4.f
constexpr float GGX_M_PI = 3.14159265359f; // common.hlsli:10, as a float

// RadicalInverse_VdC / Hammersley (:43-54)
LMX_HD float ggx_radical_inverse(uint32_t bits) {
	bits = (bits << 16u) | (bits >> 16u);
	bits = ((bits & 0x55555555u) << 1u) | ((bits & 0xAAAAAAAAu) >> 1u);
	bits = ((bits & 0x33333333u) << 2u) | ((bits & 0xCCCCCCCCu) >> 2u);
	bits = ((bits & 0x0F0F0F0Fu) << 4u) | ((bits & 0xF0F0F0F0u) >> 4u);
	bits = ((bits & 0x00FF00FFu) << 8u) | ((bits & 0xFF00FF00u) >> 8u);
	return (float)bits * 2.3283064365386963e-10f;
}

// ImportanceSampleGGX's tangent-space H (:57-67) of sample i at `roughness`: host only, libm's cosf / sinf. It depends on neither texel nor probe.
inline V3 ggx_sample_h(uint32_t i, float roughness) {
	const float xi_x = (float)i / (float)GGX_SAMPLES, xi_y = ggx_radical_inverse(i);
	const float a = roughness * roughness;
	const float phi = 2.0f * GGX_M_PI * xi_x;
	const float cos_theta = sqrtf((1.0f - xi_y) / (1.0f + (a * a - 1.0f) * xi_y));
	const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
	return V3{cosf(phi) * sin_theta, sinf(phi) * sin_theta, cos_theta};
}

// D_GGX (common.hlsli:764-769)
LMX_HD float ggx_d(float ndoth, float roughness) {
	const float a = roughness * roughness;
	const float a2 = a * a;
	const float f0 = (ndoth * ndoth) * (a2 - 1.f) + 1.f;
	const float f = 1e-5f > f0 ? 1e-5f : f0;
	return a2 / (f * f * GGX_M_PI);
}

// prefilteredImportanceSampling (:29-40) with its hard-coded dim = 128 whatever the cubemap's size is; `log2_of` is the caller's log2
LMX_HD float ggx_lod_argument(float ipdf) {
	const float inv_num_samples = 1.0f / (float)GGX_SAMPLES;
	const float dim = 128.f;
	const float omega_p = (4.0f * GGX_M_PI) / (6.0f * dim * dim);
	const float inv_omega_p = 1.0f / omega_p;
	const float omega_s = inv_num_samples * ipdf;
	return 4.0f * omega_s * inv_omega_p;
}
LMX_HD float ggx_lod_clamp(float log2_value) {
	const float l = log2_value * 0.5f;
	return l > 0.f ? (l < 4.f ? l : 4.f) : 0.f; // clamp(.., 0, 4); NaN gives 0
}

// One sample of mainPS's loop (:103-112) for the normalized N (= R = V) and the tangent-space H of the table.
struct GgxSample {
	V3 L;
	float ndotl, lod_argument; // the gate is ndotl > 0; lod = ggx_lod_clamp(log2(lod_argument))
};
LMX_HD GgxSample ggx_sample(V3 N, V3 Ht, float roughness) {
	const V3 up = abs_f(N.z) < 0.999f ? V3{0.f, 0.f, 1.f} : V3{1.f, 0.f, 0.f};
	const V3 tangent = normalize(cross(up, N));
	const V3 bitangent = cross(N, tangent);
	const V3 sv = V3{tangent.x * Ht.x + bitangent.x * Ht.y + N.x * Ht.z, tangent.y * Ht.x + bitangent.y * Ht.y + N.y * Ht.z, tangent.z * Ht.x + bitangent.z * Ht.y + N.z * Ht.z};
	const V3 H = normalize(sv);
	const float k = 2.0f * dot(N, H);
	GgxSample r;
	r.L = normalize(V3{k * H.x - N.x, k * H.y - N.y, k * H.z - N.z});
	r.ndotl = dot(N, r.L);
	const float ldoth = dot(r.L, H), ndoth = dot(N, H);
	const float ipdf = (4.0f * ldoth) / (ggx_d(ndoth, roughness) * ndoth);
	r.lod_argument = ggx_lod_argument(ipdf);
	return r;
}

// ---- RGBM (saveCubemap's loop, :3555-3559) ---------------------------------------------------------------------------------------------------
LMX_HD float rgbm_max(float a, float b) { return a > b ? a : b; } // core/math.h: maximum, minimum, clamp = minimum(maximum(v, lo), hi)
LMX_HD float rgbm_min(float a, float b) { return a < b ? a : b; }
LMX_HD float rgbm_clamp(float v, float lo, float hi) { return rgbm_min(rgbm_max(v, lo), hi); }
LMX_HD void rgbm_encode(float x, float y, float z, uint8_t out[4]) {
	const float m = rgbm_clamp(maximum3(x, y, z), 1 / 64.f, 4.f);
	out[0] = (uint8_t)rgbm_clamp(x / m * 255 + 0.5f, 0.f, 255.f);
	out[1] = (uint8_t)rgbm_clamp(y / m * 255 + 0.5f, 0.f, 255.f);
	out[2] = (uint8_t)rgbm_clamp(z / m * 255 + 0.5f, 0.f, 255.f);
	out[3] = (uint8_t)rgbm_clamp(255.f * m / 4 + 0.5f, 1.f, 255.f);
}

// ---- layout --------------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t PROBES_MAX_BATCH_BYTES = 1ull << 30; // LMX_PROBES_MAX_BATCH_BYTES: a batch of cubemaps above this is refused
constexpr uint32_t PROBES_MAX_SIZE = 4096;              // 6 * 4096^2 * 16 bytes is above the cap already; keeps every product below inside 64 bits

// texels of one cubemap's mip 0; 0 where S is 0 or above PROBES_MAX_SIZE
LMX_HD uint64_t probe_texels(uint32_t S) { return S == 0 || S > PROBES_MAX_SIZE ? 0 : 6ull * S * S; }
// bytes of a batch of n cubemaps of size S; 0 where it is empty or above the cap
LMX_HD uint64_t probe_batch_bytes(uint32_t n, uint32_t S) {
	const uint64_t one = probe_texels(S) * 16ull;
	if (one == 0 || n == 0 || one > PROBES_MAX_BATCH_BYTES || n > PROBES_MAX_BATCH_BYTES / one) return 0;
	return one * n;
}
LMX_HD bool probe_is_pow2(uint32_t S) { return S != 0 && (S & (S - 1)) == 0; }
// mips 1 .. log2 S of one cubemap, face-major inside a mip: the texels in front of mip `m` (m >= 1) and all of them (m = log2 S + 1)
LMX_HD uint64_t probe_mip_offset(uint32_t S, uint32_t m) {
	uint64_t at = 0;
	for (uint32_t k = 1; k < m; ++k) at += 6ull * (S >> k) * (S >> k);
	return at;
}
// the filtered floats of one cubemap, level-major: levels 0 .. 4 of [6][s][s][4], s = S >> level. The texels in front of `level` (5: all).
LMX_HD uint64_t probe_level_offset(uint32_t S, uint32_t level) {
	uint64_t at = 0;
	for (uint32_t k = 0; k < level; ++k) at += 6ull * (S >> k) * (S >> k);
	return at;
}
// the RGBM bytes of one cubemap, as saveCubemap's loop feeds the compressor: per face, levels 0 .. 4. The texels in front of (face, level).
LMX_HD uint64_t probe_rgbm_offset(uint32_t S, uint32_t face, uint32_t level) { return (probe_level_offset(S, GGX_LEVELS) / 6) * face + probe_level_offset(S, level) / 6; }
LMX_HD uint32_t probe_log2(uint32_t S) {
	uint32_t l = 0;
	while ((S >> l) > 1) ++l;
	return l;
}

#if defined(__HIPCC__)
// ---- probe_kernels.hip -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t PROBE_BLOCK = 256;
constexpr uint32_t SH_CHUNK = 256;  // pixels a block of k_sh_accumulate stages at a time: one per lane
constexpr uint32_t SH_STRIDE = 29;  // floats per staged pixel: 27 terms and the weight, padded to an odd stride (no bank conflicts when 64 lanes write their rows)

// table[r * n_pix + pix], r < SH_TABLE_ROWS, n_pix = 6 S^2
hipError_t launch_sh_table(hipStream_t s, uint32_t S, float* table);
// rgba: n cubemaps of float[6][S][S][4]; out: float[n][9][3]
hipError_t launch_sh_accumulate(hipStream_t s, const float* rgba, const float* table, uint32_t n, uint32_t S, float* out);
// mips: per probe probe_mip_offset(S, log2 S + 1) texels of four floats
hipError_t launch_probe_mips(hipStream_t s, const float* rgba, uint32_t n, uint32_t S, float* mips);
// the chain of a batch as the sampler reads it: mip 0 in `rgba`, mips 1 .. last_mip in `mips` (launch_probe_mips' layout)
struct ProbeChain {
	const float* rgba;
	const float* mips;
	uint32_t n, S, last_mip;
};
// ggx: the table of lmx_probes_ggx_samples, float[GGX_LEVELS][GGX_SAMPLES][3]; filtered: per probe probe_level_offset(S, 5) texels of four floats
hipError_t launch_probe_filter(hipStream_t s, const ProbeChain& chain, const float* ggx, float* filtered);
// rgbm: per probe probe_level_offset(S, 5) texels of four bytes, probe_rgbm_offset's layout
hipError_t launch_probe_rgbm(hipStream_t s, const float* filtered, uint32_t n, uint32_t S, uint8_t* rgbm);
// out[i] = cube_sample(dirs[i], lods[i]) of cubemap `probe`: three floats each
hipError_t launch_probe_sample(hipStream_t s, const ProbeChain& chain, uint32_t probe, const float* dirs, const float* lods, uint32_t n, float* out);
#endif

} // namespace lmx
