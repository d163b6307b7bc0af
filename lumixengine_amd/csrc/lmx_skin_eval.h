// lmx_skin_eval.h — evaluateSkin / Model::evalVertexPose (renderer/model.cpp:103-129) read from the palette lmx_skin_run leaves: the one
// statement of the palette layout outside skin_kernels.hip. Shared by the ray cast's narrow phase (ray_kernels.hip: the whole point) and
// the particle VM's MESH instruction (particle_kernels.hip: one component of it). FMA-free (-ffp-contract=off).
//
// `pal` = the instance's palette, 3 x float4 per bone: P0 = (m00 m01 m10 m11), P1 = (m20 m21 m30 m31) with mCR = columns[C] row R,
// P2 = row 2 = (m02 m12 m22 m32) (skin_kernels.hip "Palette layout"). The blend is ((M0 * w.x + M1 * w.y) + M2 * w.z) + M3 * w.w element by
// element (math.cpp:1022-1071), then transformPoint (math.cpp:1231-1235). A bone index past the pose reads bone 0 (the reference reads an
// uninitialised matrix there).
#pragma once

#include "lmx_kernels.h"

namespace lmx {

__device__ __forceinline__ V3 skin_point(const float4* pal, uint32_t n_bones, const LmxSkin& s, V3 p) {
	float4 a[4], b[4], c[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		uint32_t bone = (uint32_t)(uint16_t)s.indices[k];
		if (bone >= n_bones) bone = 0;
		a[k] = pal[3 * bone];
		b[k] = pal[3 * bone + 1];
		c[k] = pal[3 * bone + 2];
	}
	const float w0 = s.weights[0], w1 = s.weights[1], w2 = s.weights[2], w3 = s.weights[3];
#define LMX_RAY_BLEND(v, f) (((v[0].f * w0 + v[1].f * w1) + v[2].f * w2) + v[3].f * w3)
	const float m00 = LMX_RAY_BLEND(a, x), m01 = LMX_RAY_BLEND(a, y), m10 = LMX_RAY_BLEND(a, z), m11 = LMX_RAY_BLEND(a, w);
	const float m20 = LMX_RAY_BLEND(b, x), m21 = LMX_RAY_BLEND(b, y), m30 = LMX_RAY_BLEND(b, z), m31 = LMX_RAY_BLEND(b, w);
	const float m02 = LMX_RAY_BLEND(c, x), m12 = LMX_RAY_BLEND(c, y), m22 = LMX_RAY_BLEND(c, z), m32 = LMX_RAY_BLEND(c, w);
#undef LMX_RAY_BLEND
	return V3{m00 * p.x + m10 * p.y + m20 * p.z + m30, m01 * p.x + m11 * p.y + m21 * p.z + m31, m02 * p.x + m12 * p.y + m22 * p.z + m32};
}

// The four elements of one bone's matrix that component `sub` (0..2) of transformPoint multiplies: (m0s, m1s, m2s, m3s). Rows 0 and 1 are
// the even and the odd floats of P0 | P1, row 2 is P2: 16 bytes of the bone's 48 are read. `pal` is the instance's first bone; the offsets
// are 32-bit (a pose has at most 196 bones).
struct SkinRow { float e[4]; };
__device__ __forceinline__ SkinRow skin_row(const float4* pal, uint32_t bone, uint32_t sub) {
	const float* f = reinterpret_cast<const float*>(pal);
	const uint32_t at = 12u * bone + (sub == 2 ? 8u : sub), step = sub == 2 ? 1u : 2u;
	return SkinRow{{f[at], f[at + step], f[at + 2u * step], f[at + 3u * step]}};
}

} // namespace lmx
