// lmx_terrain_height.h — both Terrain::getHeight (renderer/terrain.cpp:402-447) on the device, shared by the terrain ray cast
// (ray_scene_kernels.hip) and the grass quads (grass_kernels.hip): one decoding of the heightmap, one interpolation. FMA-free like
// every file that includes it (-ffp-contract=off); the division is the IEEE one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmx_types.h"

namespace lmx {

__device__ __forceinline__ int32_t clamp_i(int32_t v, int32_t lo, int32_t hi) {                     // core/math.h:520-522
	const int32_t m = v > lo ? v : lo;
	return m < hi ? m : hi;
}

// (int)v as x86's cvttss2si gives it: NaN and values outside int32 are INT32_MIN (lmx::trunc_i32 for floats)
__device__ __forceinline__ int32_t trunc_i32f(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u; }

struct TerrainView { const uint8_t* texels; int32_t w, h; uint32_t format; float sx, sy, sz; };

// Terrain::getHeight(int, int), terrain.cpp:430-447
__device__ __forceinline__ float terrain_texel_height(const TerrainView& tv, int32_t x, int32_t z) {
	const float DIV64K = 1.0f / 65535.0f;
	const float DIV255 = 1.0f / 255.0f;
	const int32_t idx = clamp_i(x, 0, tv.w - 1) + clamp_i(z, 0, tv.h - 1) * tv.w; // (>= 0 and < w * h <= 2^30: checked when the table was set)
	if (tv.format == LMX_RAY_TERRAIN_R16) return tv.sy * DIV64K * (float)(int32_t)reinterpret_cast<const uint16_t*>(tv.texels)[idx];
	return tv.sy * DIV255 * (float)(reinterpret_cast<const uint32_t*>(tv.texels)[idx] & 0xffu);
}

// Terrain::getHeight(float, float), terrain.cpp:402-427
__device__ __forceinline__ float terrain_height(const TerrainView& tv, float x, float z) {
	const float inv_scale = 1.0f / tv.sx;
	const int32_t int_x = trunc_i32f(x * inv_scale);
	const int32_t int_z = trunc_i32f(z * inv_scale);
	const float dec_x = (x - ((float)int_x * tv.sx)) * inv_scale;
	const float dec_z = (z - ((float)int_z * tv.sx)) * inv_scale;
	if (dec_z == 0 && dec_x == 0) return terrain_texel_height(tv, int_x, int_z);
	if (dec_x > dec_z) {
		const float h0 = terrain_texel_height(tv, int_x, int_z);
		const float h1 = terrain_texel_height(tv, int_x + 1, int_z);
		const float h2 = terrain_texel_height(tv, int_x + 1, int_z + 1);
		return h0 + (h1 - h0) * dec_x + (h2 - h1) * dec_z;
	}
	const float h0 = terrain_texel_height(tv, int_x, int_z);
	const float h1 = terrain_texel_height(tv, int_x + 1, int_z + 1);
	const float h2 = terrain_texel_height(tv, int_x, int_z + 1);
	return h0 + (h2 - h0) * dec_z + (h1 - h2) * dec_x;
}

} // namespace lmx
