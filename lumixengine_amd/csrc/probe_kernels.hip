// probe_kernels.hip — the probe bake (EnvironmentProbePlugin, renderer/editor/render_plugins.cpp) on the device. The arithmetic is
// lmx_probes.h's, shared with the host; FMA-free (-ffp-contract=off), so coefficients, mip texels and RGBM bytes equal the reference's bit for
// bit; the radiance levels are held to a bound (their sum order is free, the device's log2 is its own).
//
//   k_sh_table       one lane per pixel of a cubemap of size S: project's nine values and the weight, table[row * n_pix + pix]. They depend
//                    on S alone; the host keeps the table while S stays.
//   k_sh_accumulate  ONE BLOCK per probe. SphericalHarmonics::compute adds its 98 304 terms (S = 128) in face, y, x order into 27 sums, and
//                    weightSum in the same order: a chain per sum that may not be reordered. The parallelism is probes x chains. The block
//                    walks the probe's pixels in chunks of SH_CHUNK: every lane takes one pixel, reads its colour and table row and stores
//                    the 27 products `b_i * (color_c * weight)` and the weight into LDS (only the add is a chain); behind a barrier lane k < 27
//                    of the first wave adds column k of the chunk in pixel order, lane 27 the weights. The last step is sh_finish.
//   k_probe_mip      one lane per texel of a mip level, all probes of the batch: the `downscale` program's sum of four, times 0.25f.
//   k_probe_level0   one lane per texel of level 0: the shader's `u_mip == 0` branch, the sampler at the texel's own direction (= mip 0).
//   k_probe_filter   levels 1 .. 4 of ibl_filter.hlsl's mainPS. ONE WAVE per output texel, the 128 samples two per lane, a wave reduction;
//                    the level's table of tangent-space H (lmx_probes_ggx_samples) staged in LDS. One launch per level.
//   k_probe_rgbm     one lane per texel of (probe, level): saveCubemap's bytes in its face-major order.
//   k_probe_sample   one lane per query: the cube sampler alone (lmx_probes_sample).
#include <hip/hip_runtime.h>

#include "lmx_probes.h"

namespace lmx {

namespace {

__global__ __launch_bounds__(PROBE_BLOCK) void k_sh_table(uint32_t S, uint32_t n_pix, float* __restrict__ table) {
	const uint32_t pix = blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if (pix >= n_pix) return;
	const uint32_t face = pix / (S * S), rest = pix % (S * S);
	const uint32_t y = rest / S, x = rest % S;
	float b[SH_COEFS];
	sh_project(sh_cube2dir(x, y, face, S), b);
	for (uint32_t i = 0; i < SH_COEFS; ++i) table[(size_t)i * n_pix + pix] = b[i];
	table[(size_t)SH_COEFS * n_pix + pix] = sh_weight(x, y, S);
}

__global__ __launch_bounds__(PROBE_BLOCK) void k_sh_accumulate(const float* __restrict__ rgba, const float* __restrict__ table, uint32_t n_pix, float* __restrict__ out) {
	__shared__ float s_term[SH_CHUNK * SH_STRIDE];
	__shared__ float s_weight_sum;
	const uint32_t probe = blockIdx.x, t = threadIdx.x;
	const float4* colours = reinterpret_cast<const float4*>(rgba) + (size_t)probe * n_pix; // (a cubemap is a multiple of 16 bytes)
	float sum = 0.f; // lane k < 27: coefs[k / 3] channel k % 3; lane 27: weightSum
	for (uint32_t base = 0; base < n_pix; base += SH_CHUNK) { // block-uniform
		const uint32_t pix = base + t;
		if (pix < n_pix) {
			const float4 c = colours[pix];
			const float w = table[(size_t)SH_COEFS * n_pix + pix];
			float* row = s_term + t * SH_STRIDE;
			for (uint32_t i = 0; i < SH_COEFS; ++i) {
				const float b = table[(size_t)i * n_pix + pix];
				row[3 * i + 0] = sh_term(b, c.x, w);
				row[3 * i + 1] = sh_term(b, c.y, w);
				row[3 * i + 2] = sh_term(b, c.z, w);
			}
			row[27] = w;
		}
		__syncthreads();
		if (t < 28) {
			const uint32_t m = n_pix - base < SH_CHUNK ? n_pix - base : SH_CHUNK;
			for (uint32_t p = 0; p < m; ++p) sum += s_term[p * SH_STRIDE + t];
		}
		__syncthreads();
	}
	if (t == 27) s_weight_sum = sum;
	__syncthreads();
	if (t < 27) out[(size_t)probe * 27 + t] = sh_finish(sum, s_weight_sum, t / 3);
}

// src: n images of [6][2 s][2 s][4] floats, src_stride floats apart; dst: n images of [6][s][s][4], dst_stride apart
__global__ __launch_bounds__(PROBE_BLOCK) void k_probe_mip(const float* __restrict__ src, size_t src_stride, float* __restrict__ dst, size_t dst_stride, uint32_t s, uint32_t n_texels) {
	const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x, probe = blockIdx.y;
	if (i >= n_texels) return; // n_texels = 6 s^2
	const uint32_t face = i / (s * s), rest = i % (s * s);
	const uint32_t y = rest / s, x = rest % s;
	const float4* in = reinterpret_cast<const float4*>(src + (size_t)probe * src_stride) + (size_t)face * (4u * s * s);
	const float4 v00 = in[(size_t)(2 * y) * (2 * s) + 2 * x], v10 = in[(size_t)(2 * y) * (2 * s) + 2 * x + 1];
	const float4 v01 = in[(size_t)(2 * y + 1) * (2 * s) + 2 * x], v11 = in[(size_t)(2 * y + 1) * (2 * s) + 2 * x + 1];
	float4 r;
	r.x = mip_average(v00.x, v10.x, v01.x, v11.x);
	r.y = mip_average(v00.y, v10.y, v01.y, v11.y);
	r.z = mip_average(v00.z, v10.z, v01.z, v11.z);
	r.w = mip_average(v00.w, v10.w, v01.w, v11.w);
	reinterpret_cast<float4*>(dst + (size_t)probe * dst_stride)[i] = r;
}

// the texel reader of cube_sample for cubemap `probe` of a chain (mip, face, x and y are inside the chain: the sampler clamps them)
struct ChainFetch {
	const float* mip0;
	const float* mips;
	uint32_t S;
	__device__ __forceinline__ ChainFetch(const ProbeChain& c, uint32_t probe)
		: mip0(c.rgba + (size_t)probe * (4 * (size_t)probe_texels(c.S))), mips(c.mips + (size_t)probe * (4 * (size_t)probe_mip_offset(c.S, c.last_mip + 1))), S(c.S) {}
	__device__ __forceinline__ V3 operator()(uint32_t mip, uint32_t face, uint32_t x, uint32_t y) const {
		const uint32_t s = S >> mip;
		const float* base = mip == 0 ? mip0 : mips + 4 * (size_t)probe_mip_offset(S, mip);
		const float4 t = reinterpret_cast<const float4*>(base)[((size_t)face * s + y) * s + x];
		return V3{t.x, t.y, t.z};
	}
};

constexpr uint32_t FILTER_TEXELS_PER_BLOCK = PROBE_BLOCK / 64;

// level 0: one lane per texel, the shader's `u_mip == 0` branch: the cubemap sampled at the texel's own direction
__global__ __launch_bounds__(PROBE_BLOCK) void k_probe_level0(ProbeChain c, float* __restrict__ filtered, size_t probe_stride) {
	const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x, probe = blockIdx.y, s = c.S;
	if (i >= 6 * s * s) return;
	const uint32_t face = i / (s * s), rest = i % (s * s);
	const V3 col = cube_sample(probe_texel_dir(rest % s, rest / s, face, s), 0.f, c.last_mip, ChainFetch(c, probe));
	reinterpret_cast<float4*>(filtered + (size_t)probe * probe_stride)[i] = make_float4(col.x, col.y, col.z, 1.f);
}

// levels 1 .. 4: ONE WAVE per output texel, the 128 samples two per lane; the table of tangent-space H of the level is staged in LDS.
__global__ __launch_bounds__(PROBE_BLOCK) void k_probe_filter(ProbeChain c, const float* __restrict__ ggx, uint32_t level, float* __restrict__ filtered, size_t probe_stride) {
	__shared__ float s_h[GGX_SAMPLES * 3];
	for (uint32_t k = threadIdx.x; k < GGX_SAMPLES * 3; k += PROBE_BLOCK) s_h[k] = ggx[level * (GGX_SAMPLES * 3) + k];
	__syncthreads();
	const uint32_t s = c.S >> level, probe = blockIdx.y;
	const uint32_t i = blockIdx.x * FILTER_TEXELS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (i >= 6 * s * s) return; // (behind the barrier; whole waves leave)
	const uint32_t face = i / (s * s), rest = i % (s * s);
	const V3 N = normalize(probe_texel_dir(rest % s, rest / s, face, s));
	const float roughness = (float)level / (float)(GGX_LEVELS - 1);
	const ChainFetch fetch(c, probe);
	float r = 0.f, g = 0.f, b = 0.f, w = 0.f;
	for (uint32_t k = lane; k < GGX_SAMPLES; k += 64) {
		const GgxSample q = ggx_sample(N, V3{s_h[3 * k], s_h[3 * k + 1], s_h[3 * k + 2]}, roughness);
		if (q.ndotl > 0.0f) {
			const V3 col = cube_sample(q.L, ggx_lod_clamp(log2f(q.lod_argument)), c.last_mip, fetch);
			r += col.x * q.ndotl;
			g += col.y * q.ndotl;
			b += col.z * q.ndotl;
			w += q.ndotl;
		}
	}
	for (int off = 32; off > 0; off >>= 1) { // (the order of this sum is free: DESIGN.md §4.22)
		r += __shfl_xor(r, off);
		g += __shfl_xor(g, off);
		b += __shfl_xor(b, off);
		w += __shfl_xor(w, off);
	}
	if (lane == 0) reinterpret_cast<float4*>(filtered + (size_t)probe * probe_stride)[probe_level_offset(c.S, level) + i] = make_float4(r / w, g / w, b / w, 1.f);
}

// one lane per texel of (probe, level): saveCubemap's bytes, face-major
__global__ __launch_bounds__(PROBE_BLOCK) void k_probe_rgbm(const float* __restrict__ filtered, uint32_t S, uint8_t* __restrict__ rgbm) {
	const uint32_t level = blockIdx.z, probe = blockIdx.y, s = S >> level;
	const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if (i >= 6 * s * s) return;
	const size_t texels = (size_t)probe_level_offset(S, GGX_LEVELS);
	const float4 t = reinterpret_cast<const float4*>(filtered)[probe * texels + probe_level_offset(S, level) + i];
	uint8_t q[4];
	rgbm_encode(t.x, t.y, t.z, q);
	const uint32_t face = i / (s * s), rest = i % (s * s);
	reinterpret_cast<uint32_t*>(rgbm)[probe * texels + probe_rgbm_offset(S, face, level) + rest] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; // r, g, b, a
}

__global__ __launch_bounds__(PROBE_BLOCK) void k_probe_sample(ProbeChain c, uint32_t probe, const float* __restrict__ dirs, const float* __restrict__ lods, uint32_t n, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if (i >= n) return;
	const V3 col = cube_sample(V3{dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]}, lods[i], c.last_mip, ChainFetch(c, probe));
	out[3 * (size_t)i] = col.x;
	out[3 * (size_t)i + 1] = col.y;
	out[3 * (size_t)i + 2] = col.z;
}

// a chain the sampler can read: a power of two of 16 or more (five levels exist), a batch inside the cap and a grid's second dimension
bool chain_ok(const ProbeChain& c) {
	return c.n != 0 && c.n <= 65535 && probe_is_pow2(c.S) && c.S >= 16 && probe_batch_bytes(c.n, c.S) != 0 && c.last_mip == probe_log2(c.S) && c.rgba && c.mips;
}

} // namespace

hipError_t launch_sh_table(hipStream_t s, uint32_t S, float* table) {
	const uint64_t n_pix = probe_texels(S);
	if (n_pix == 0 || n_pix > 0x7fffffffull) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_sh_table, dim3((uint32_t)((n_pix + PROBE_BLOCK - 1) / PROBE_BLOCK)), dim3(PROBE_BLOCK), 0, s, S, (uint32_t)n_pix, table);
	return hipGetLastError();
}

hipError_t launch_sh_accumulate(hipStream_t s, const float* rgba, const float* table, uint32_t n, uint32_t S, float* out) {
	const uint64_t n_pix = probe_texels(S);
	if (n == 0 || probe_batch_bytes(n, S) == 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_sh_accumulate, dim3(n), dim3(PROBE_BLOCK), 0, s, rgba, table, (uint32_t)n_pix, out);
	return hipGetLastError();
}

hipError_t launch_probe_mips(hipStream_t s, const float* rgba, uint32_t n, uint32_t S, float* mips) {
	if (n == 0 || n > 65535 || !probe_is_pow2(S) || S < 2 || probe_batch_bytes(n, S) == 0) return hipErrorInvalidValue;
	const uint32_t levels = probe_log2(S);
	const size_t mip_stride = 4 * (size_t)probe_mip_offset(S, levels + 1);
	for (uint32_t m = 1; m <= levels; ++m) {
		const uint32_t sz = S >> m, n_texels = 6 * sz * sz;
		const float* src = m == 1 ? rgba : mips + 4 * (size_t)probe_mip_offset(S, m - 1);
		const size_t src_stride = m == 1 ? 4 * (size_t)probe_texels(S) : mip_stride;
		hipLaunchKernelGGL(k_probe_mip, dim3((n_texels + PROBE_BLOCK - 1) / PROBE_BLOCK, n), dim3(PROBE_BLOCK), 0, s, src, src_stride, mips + 4 * (size_t)probe_mip_offset(S, m), mip_stride, sz, n_texels);
		if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launch_probe_filter(hipStream_t s, const ProbeChain& chain, const float* ggx, float* filtered) {
	if (!chain_ok(chain)) return hipErrorInvalidValue;
	const size_t stride = 4 * (size_t)probe_level_offset(chain.S, GGX_LEVELS);
	hipLaunchKernelGGL(k_probe_level0, dim3((6 * chain.S * chain.S + PROBE_BLOCK - 1) / PROBE_BLOCK, chain.n), dim3(PROBE_BLOCK), 0, s, chain, filtered, stride);
	if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
	for (uint32_t level = 1; level < GGX_LEVELS; ++level) {
		const uint32_t sz = chain.S >> level, n_texels = 6 * sz * sz;
		hipLaunchKernelGGL(k_probe_filter, dim3((n_texels + FILTER_TEXELS_PER_BLOCK - 1) / FILTER_TEXELS_PER_BLOCK, chain.n), dim3(PROBE_BLOCK), 0, s, chain, ggx, level, filtered, stride);
		if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launch_probe_rgbm(hipStream_t s, const float* filtered, uint32_t n, uint32_t S, uint8_t* rgbm) {
	if (n == 0 || n > 65535 || !probe_is_pow2(S) || S < 16 || probe_batch_bytes(n, S) == 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_probe_rgbm, dim3((6 * S * S + PROBE_BLOCK - 1) / PROBE_BLOCK, n, GGX_LEVELS), dim3(PROBE_BLOCK), 0, s, filtered, S, rgbm);
	return hipGetLastError();
}

hipError_t launch_probe_sample(hipStream_t s, const ProbeChain& chain, uint32_t probe, const float* dirs, const float* lods, uint32_t n, float* out) {
	if (n == 0) return hipSuccess;
	if (!chain_ok(chain) || probe >= chain.n) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_probe_sample, dim3((n + PROBE_BLOCK - 1) / PROBE_BLOCK), dim3(PROBE_BLOCK), 0, s, chain, probe, dirs, lods, n, out);
	return hipGetLastError();
}

} // namespace lmx
