// lmx_cluster_planes.cpp — host mirror of the cluster planes PipelineImpl::fillClusters builds per view (renderer/pipeline.cpp:3464-3495),
// next to lmx_frustum.cpp: per view, not per light. The z planes take libm's powf - the device's is not the same function, and one
// differing last bit in a z plane moves lights across cluster borders - so the kernels receive the finished planes. Operation order as in
// the reference (lerp core/math.cpp:194-201, cross :1274-1276, normalize :367-376, makePlane core/geometry.cpp:820-824). Compiled with
// -ffp-contract=off.
#include <cmath>
#include <cstring>

#include "lumix_mi355.h"
#include "lmx_math.h"

using namespace lmx;

namespace {

V3 normalize3(V3 v) { // core/math.cpp:367-376
	float x = v.x, y = v.y, z = v.z;
	const float inv_len = 1 / sqrtf(x * x + y * y + z * z);
	x *= inv_len;
	y *= inv_len;
	z *= inv_len;
	return V3{x, y, z};
}

V3 lerp3(V3 a, V3 b, float t) { // core/math.cpp:194-201
	const float invt = 1.0f - t;
	return V3{a.x * invt + b.x * t, a.y * invt + b.y * t, a.z * invt + b.z * t};
}

void make_plane(float out[4], V3 normal, V3 point) { // core/geometry.cpp:820-824
	out[0] = normal.x;
	out[1] = normal.y;
	out[2] = normal.z;
	out[3] = -dot(normal, point);
}

// libm's powf at run time, as the engine calls it: through a volatile pointer, so that no compiler folds the 17 constant calls with an
// evaluation of its own
float (*volatile libm_powf)(float, float) = powf;

} // namespace

extern "C" int lmx_clusters_planes(const LmxShiftedFrustum* frustum, uint32_t viewport_w, uint32_t viewport_h, LmxClusterPlanes* out) {
	if (!frustum || !out) return LMX_ERR_INVALID_ARGUMENT;
	const uint64_t sx = ((uint64_t)viewport_w + 63) / 64, sy = ((uint64_t)viewport_h + 63) / 64;
	if (sx > LMX_CLUSTER_MAX_XY || sy > LMX_CLUSTER_MAX_XY) return LMX_ERR_CAPACITY; // Vec4 xplanes[65], yplanes[65] (:3464-3465)
	memset(out, 0, sizeof(*out));
	const int size_x = (int)sx, size_y = (int)sy, size_z = LMX_CLUSTER_Z;
	out->size[0] = (uint32_t)size_x;
	out->size[1] = (uint32_t)size_y;
	out->size[2] = (uint32_t)size_z;
	V3 p[8];
	for (int i = 0; i < 8; ++i) p[i] = V3{frustum->points[i][0], frustum->points[i][1], frustum->points[i][2]};

	const V3 cam_dir = normalize3(cross(sub(p[2], p[0]), sub(p[1], p[0])));
	for (int i = 0; i < size_z + 1; ++i) {
		const float znear = 0.1f;
		const float zfar = 10000.0f;
		const float z = znear * libm_powf(zfar / znear, i / (float)size_z);
		make_plane(out->zplanes[i], cam_dir, mul(cam_dir, z));
	}
	for (int i = 0; i < size_y + 1; ++i) {
		const float t = i / (float)size_y;
		const V3 a = lerp3(p[0], p[3], t);
		const V3 b = lerp3(p[1], p[2], t);
		const V3 c = lerp3(p[4], p[7], t);
		make_plane(out->yplanes[i], normalize3(cross(sub(b, a), sub(c, a))), a);
	}
	for (int i = 0; i < size_x + 1; ++i) {
		const float t = i / (float)size_x;
		const V3 a = lerp3(p[1], p[0], t);
		const V3 b = lerp3(p[2], p[3], t);
		const V3 c = lerp3(p[5], p[4], t);
		make_plane(out->xplanes[i], normalize3(cross(sub(b, a), sub(c, a))), a);
	}
	return LMX_OK;
}
