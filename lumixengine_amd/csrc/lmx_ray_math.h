// lmx_ray_math.h — the device arithmetic every ray-cast stage shares (ray_kernels.hip, ray_scene_kernels.hip): the reference's ray / AABB and
// ray / triangle tests in its operation order, the ordered 64-bit keys of the atomic minima and the candidate count. One copy: a stage that
// re-tests a winning triangle gets the narrow phase's bits because it runs the narrow phase's statements. FMA-free (-ffp-contract=off).
#pragma once

#include "lmx_kernels.h"

namespace lmx {

__device__ __forceinline__ float safe_inverse_scale(float v) { return v == 0.0f ? 0.0f : 1.0f / v; } // core/math.cpp:9-12
__device__ __forceinline__ float minimum(float a, float b) { return a < b ? a : b; }               // core/math.h:420-422
__device__ __forceinline__ float maximum(float a, float b) { return a > b ? a : b; }               // core/math.h:472-475

// getRayAABBIntersection(origin, dir, min, size, out), core/geometry.cpp:861-889; `mx` = min + size as the function forms it. *tmin_out:
// out = tmin < 0 ? origin : origin + dir * tmin is left to the caller
__device__ __forceinline__ bool ray_aabb_tmin(V3 o, V3 dir, V3 mn, V3 mx, float* tmin_out) {
	const float fx = 1.0f / (dir.x == 0 ? 0.00000001f : dir.x);
	const float fy = 1.0f / (dir.y == 0 ? 0.00000001f : dir.y);
	const float fz = 1.0f / (dir.z == 0 ? 0.00000001f : dir.z);
	const float t1 = (mn.x - o.x) * fx, t2 = (mx.x - o.x) * fx;
	const float t3 = (mn.y - o.y) * fy, t4 = (mx.y - o.y) * fy;
	const float t5 = (mn.z - o.z) * fz, t6 = (mx.z - o.z) * fz;
	const float tmin = maximum(maximum(minimum(t1, t2), minimum(t3, t4)), minimum(t5, t6));
	const float tmax = minimum(minimum(maximum(t1, t2), maximum(t3, t4)), maximum(t5, t6));
	if (tmax < 0) return false;
	if (tmin > tmax) return false;
	*tmin_out = tmin;
	return true;
}
__device__ __forceinline__ bool ray_aabb(V3 o, V3 dir, V3 mn, V3 mx) {
	float tmin;
	return ray_aabb_tmin(o, dir, mn, mx, &tmin);
}

// getRayTriangleIntersection, core/geometry.cpp:927-967, textually the triangle test of Model::castRay, model.cpp:186-206. A NaN t is no
// hit (the reference accepts it as a first hit).
__device__ __forceinline__ bool ray_triangle(V3 p0, V3 p1, V3 p2, V3 origin, V3 dir, float* out_t) {
	const V3 normal = cross(sub(p1, p0), sub(p2, p0));
	const float q = dot(normal, dir);
	if (q == 0) return false;
	const float dd = -dot(normal, p0);
	const float t = -(dot(normal, origin) + dd) / q;
	if (t < 0) return false;
	if (t != t) return false;
	const V3 hit_point = add(origin, mul(dir, t));
	if (dot(normal, cross(sub(p1, p0), sub(hit_point, p0))) < 0) return false;
	if (dot(normal, cross(sub(p2, p1), sub(hit_point, p1))) < 0) return false;
	if (dot(normal, cross(sub(p0, p2), sub(hit_point, p2))) < 0) return false;
	*out_t = t;
	return true;
}

// (t bits << 32) | index that orders as `<` does over every non-NaN t, negative ones included; -0 as +0
__device__ __forceinline__ unsigned long long ordered_key(float t, uint32_t index) {
	const uint32_t bits = t == 0 ? 0u : __float_as_uint(t);
	const uint32_t ordered = (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
	return (unsigned long long)ordered << 32 | index;
}

// candidates on the list of the stage whose state words `d` carries: its cursor, capped at the reserve
__device__ __forceinline__ uint32_t candidates(const RaysDevice& d) {
	const unsigned long long n = *reinterpret_cast<const unsigned long long*>(d.state + RAYS_COUNTER);
	return n < d.max_cand ? (uint32_t)n : d.max_cand;
}

} // namespace lmx
