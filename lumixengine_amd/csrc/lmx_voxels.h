// lmx_voxels.h — the arithmetic of Voxels (renderer/voxels.cpp), shared by voxel_kernels.hip and the host side of lmx_capi_voxels.hip:
// beginRaster's grid, raster's cell box and box/triangle test (core/geometry.cpp:1007-1066), the generator of core/math.cpp:1337-1378 with
// its closed-form skip, castRay's march, the point lookup and the importer's u8 bake. FMA-free fp32 in the reference's operation order
// (-ffp-contract=off); nothing here may be reassociated. The launchers of the four kernels are declared at the end.
#pragma once

#include "lmx_math.h"

namespace lmx {

struct VoxelGrid {
	float mn[3], mx[3]; // m_aabb (the caller's box grown by 1.5 voxels on both sides)
	float voxel_size;
	int32_t res[3];     // m_grid_resolution
};

LMX_HD float vx_min(float a, float b) { return a < b ? a : b; }                    // core/math.h: minimum
LMX_HD float vx_max(float a, float b) { return a > b ? a : b; }                    // ... maximum
LMX_HD float vx_min3(float a, float b, float c) { return vx_min(a, vx_min(b, c)); } // the variadic forms fold from the right
LMX_HD float vx_max3(float a, float b, float c) { return vx_max(a, vx_max(b, c)); }

// int(float) as g++ compiles it for x86-64 (cvttss2si): truncation toward zero; NaN and values outside the i32 range give INT32_MIN
LMX_HD int32_t vx_i32(float v) {
	if (v > -2147483904.0f && v < 2147483648.0f) return (int32_t)v;
	return (int32_t)0x80000000u;
}

// Voxels::beginRaster (voxels.cpp:172-185). The quotient max_extent / max_res and the three resolutions are true divisions.
LMX_HD VoxelGrid voxel_grid(const float aabb_min[3], const float aabb_max[3], uint32_t max_res) {
	VoxelGrid g;
	const float vs = vx_max3(aabb_max[0] - aabb_min[0], aabb_max[1] - aabb_min[1], aabb_max[2] - aabb_min[2]) / (float)max_res;
	const float margin = vs * 1.5f;
	for (int k = 0; k < 3; ++k) {
		g.mn[k] = aabb_min[k] - margin;
		g.mx[k] = aabb_max[k] + margin;
	}
	for (int k = 0; k < 3; ++k) g.res[k] = vx_i32((g.mx[k] - g.mn[k]) / vs);
	g.voxel_size = vs;
	return g;
}

LMX_HD uint64_t voxel_cells(const VoxelGrid& g) { return (uint64_t)(uint32_t)g.res[0] * (uint32_t)g.res[1] * (uint32_t)g.res[2]; } // (res >= 0 where a grid was accepted)
LMX_HD uint32_t voxel_index(const VoxelGrid& g, int32_t x, int32_t y, int32_t z) { return (uint32_t)(x + (y + z * g.res[1]) * g.res[0]); }

// raster's to_grid (voxels.cpp:188-190): Vec3::operator/(float) multiplies by 1 / s; IVec3(Vec3) truncates
LMX_HD IV3 voxel_to_grid(const VoxelGrid& g, V3 p) {
	const float tmp = 1 / g.voxel_size;
	return IV3{vx_i32((p.x - g.mn[0]) * tmp + 0.5f), vx_i32((p.y - g.mn[1]) * tmp + 0.5f), vx_i32((p.z - g.mn[2]) * tmp + 0.5f)};
}

// the cell box of a triangle (voxels.cpp:211-217): AABB::addPoint's fold, one voxel of slack below
struct VoxelBox { IV3 lo, hi; };
LMX_HD VoxelBox voxel_triangle_box(const VoxelGrid& g, V3 p0, V3 p1, V3 p2) {
	V3 mn = p0, mx = p0;
	mn = V3{vx_min(p1.x, mn.x), vx_min(p1.y, mn.y), vx_min(p1.z, mn.z)};
	mx = V3{vx_max(p1.x, mx.x), vx_max(p1.y, mx.y), vx_max(p1.z, mx.z)};
	mn = V3{vx_min(p2.x, mn.x), vx_min(p2.y, mn.y), vx_min(p2.z, mn.z)};
	mx = V3{vx_max(p2.x, mx.x), vx_max(p2.y, mx.y), vx_max(p2.z, mx.z)};
	VoxelBox b;
	b.lo = voxel_to_grid(g, V3{mn.x - g.voxel_size, mn.y - g.voxel_size, mn.z - g.voxel_size});
	b.hi = voxel_to_grid(g, mx);
	return b;
}
// ... cut to the grid: setVoxel skips every other cell (voxels.cpp:202-209). `n` = cells left, 0 for an empty box.
struct VoxelSpan { int32_t lo[3]; uint32_t ext[3]; uint64_t n; };
LMX_HD VoxelSpan voxel_clip_box(const VoxelGrid& g, const VoxelBox& b) {
	const int32_t lo[3] = {b.lo.x, b.lo.y, b.lo.z}, hi[3] = {b.hi.x, b.hi.y, b.hi.z};
	VoxelSpan s;
	s.n = 1;
	for (int k = 0; k < 3; ++k) {
		const int32_t l = lo[k] > 0 ? lo[k] : 0, h = hi[k] < g.res[k] - 1 ? hi[k] : g.res[k] - 1;
		s.lo[k] = l;
		s.ext[k] = h >= l ? (uint32_t)(h - l) + 1u : 0u;
		s.n *= s.ext[k];
	}
	return s;
}

// testAABBTriangleCollision (core/geometry.cpp:1007-1066) on the box raster's `intersect` builds for a cell (voxels.cpp:192-200): the nine
// cross axes us x es, the three box axes, the plane with its two comparisons. The products by the unit vectors' zeros and ones are kept:
// they decide the sign of a zero and turn an infinity into a NaN exactly where the reference's do.
LMX_HD bool voxel_cell_hits_triangle(const VoxelGrid& g, int32_t i, int32_t j, int32_t k, V3 a, V3 b, V3 c) {
	const float vs = g.voxel_size;
	const float hv = 0.5f * vs;
	const V3 center = V3{(float)i * vs + hv + g.mn[0], (float)j * vs + hv + g.mn[1], (float)k * vs + hv + g.mn[2]}; // from_grid
	const V3 bmin = V3{center.x - hv, center.y - hv, center.z - hv}, bmax = V3{center.x + hv, center.y + hv, center.z + hv};
	const V3 aabbcenter = mul(add(bmax, bmin), 0.5f);
	const V3 half = mul(sub(bmax, bmin), 0.5f);
	const V3 v1 = sub(a, aabbcenter), v2 = sub(b, aabbcenter), v3_ = sub(c, aabbcenter);
	const V3 us[3] = {V3{1, 0, 0}, V3{0, 1, 0}, V3{0, 0, 1}};
	const V3 es[3] = {sub(v2, v1), sub(v3_, v2), sub(v1, v3_)};
	for (int ui = 0; ui < 3; ++ui) {
		for (int ei = 0; ei < 3; ++ei) {
			const V3 n = cross(us[ui], es[ei]);
			const float p0 = dot(v1, n), p1 = dot(v2, n), p2 = dot(v3_, n);
			const float r = dot(half, V3{fabsf(n.x), fabsf(n.y), fabsf(n.z)});
			if (vx_max(-vx_max3(p0, p1, p2), vx_min3(p0, p1, p2)) > r) return false;
		}
	}
	float mn = vx_min3(v1.x, v2.x, v3_.x), mx = vx_max3(v1.x, v2.x, v3_.x);
	if (mn > half.x || mx < -half.x) return false;
	mn = vx_min3(v1.y, v2.y, v3_.y); mx = vx_max3(v1.y, v2.y, v3_.y);
	if (mn > half.y || mx < -half.y) return false;
	mn = vx_min3(v1.z, v2.z, v3_.z); mx = vx_max3(v1.z, v2.z, v3_.z);
	if (mn > half.z || mx < -half.z) return false;
	const V3 normal = cross(es[0], es[1]);
	const float d = dot(normal, v1);
	const V3 vmin = V3{normal.x > 0.0f ? -half.x : half.x, normal.y > 0.0f ? -half.y : half.y, normal.z > 0.0f ? -half.z : half.z};
	if (dot(normal, vmin) > d) return false;
	return -dot(normal, vmin) >= d;
}

// ---- RandomGenerator (core/math.cpp:1337-1378) ---------------------------------------------------------------------------------------
// Each half is a multiply-with-carry step x <- a (x & 65535) + (x >> 16). With m = a 2^16 - 1 the step multiplies by 2^-16 = a modulo m:
// from the second step on the state lies in [1, m] (0 stays 0; m, the residue 0, is the other fixed point) and the congruence names it.
constexpr uint32_t VOXEL_RNG_A_U = 36969u, VOXEL_RNG_A_V = 18000u;
constexpr uint64_t VOXEL_RNG_M_U = 36969ull * 65536ull - 1ull; // 2422800383
constexpr uint64_t VOXEL_RNG_M_V = 18000ull * 65536ull - 1ull; // 1179647999

template <uint32_t A> LMX_HD uint32_t voxel_rng_step(uint32_t x) { return A * (x & 65535u) + (x >> 16); }
template <uint64_t M> LMX_HD uint32_t voxel_rng_canon(uint64_t r) { return r == 0 ? (uint32_t)M : (uint32_t)r; }
// a canonical state (two or more steps behind the seed) times a^k: `ak` = a^k mod m
template <uint64_t M> LMX_HD uint32_t voxel_rng_mul(uint32_t x, uint32_t ak) { return voxel_rng_canon<M>((uint64_t)x * ak % M); }
template <uint32_t A, uint64_t M> LMX_HD uint32_t voxel_rng_pow(uint64_t k) { // a^k mod m
	uint64_t r = 1, b = A;
	while (k) {
		if (k & 1) r = r * b % M;
		b = b * b % M;
		k >>= 1;
	}
	return (uint32_t)r;
}
// the state n steps behind x: the first two steps as the generator takes them, the rest in one jump
template <uint32_t A, uint64_t M> LMX_HD uint32_t voxel_rng_skip_half(uint32_t x, uint64_t n) {
	if (n == 0) return x;
	x = voxel_rng_step<A>(x);
	if (n == 1) return x;
	x = voxel_rng_step<A>(x);
	if (n == 2 || x == 0) return x;
	return voxel_rng_mul<M>(x, voxel_rng_pow<A, M>(n - 2));
}
struct VoxelRng {
	uint32_t u, v;
	LMX_HD uint32_t rand() {
		u = voxel_rng_step<VOXEL_RNG_A_U>(u);
		v = voxel_rng_step<VOXEL_RNG_A_V>(v);
		return (u << 16) + v;
	}
	LMX_HD float rand_float() { return (float)((double)rand() * 2.328306435996595e-10); } // an fp64 product rounded to fp32
};
LMX_HD VoxelRng voxel_rng_skip(VoxelRng s, uint64_t n) {
	return VoxelRng{voxel_rng_skip_half<VOXEL_RNG_A_U, VOXEL_RNG_M_U>(s.u, n), voxel_rng_skip_half<VOXEL_RNG_A_V, VOXEL_RNG_M_V>(s.v, n)};
}

// One ray of computeAO (voxels.cpp:129-133): three draws, `Vec3(randFloat(), randFloat(), randFloat())` evaluated right to left as g++
// evaluates it (the first draw is z), * 2 - 1, times the reciprocal of the largest magnitude.
LMX_HD V3 voxel_ray_dir(VoxelRng& rng) {
	const float rz = rng.rand_float();
	const float ry = rng.rand_float();
	const float rx = rng.rand_float();
	V3 dir = V3{rx * 2.f - 1.f, ry * 2.f - 1.f, rz * 2.f - 1.f};
	const float inv = 1.0f / vx_max3(fabsf(dir.x), fabsf(dir.y), fabsf(dir.z));
	dir.x *= inv; dir.y *= inv; dir.z *= inv;
	return dir;
}

// castRay (voxels.cpp:82-95) from the voxel's centre plus dir (:131-132); `occupied(linear index)` reads the grid
template <typename F> LMX_HD bool voxel_cast_ray(const VoxelGrid& g, int32_t x, int32_t y, int32_t z, V3 d, const F& occupied) {
	const V3 s = V3{(float)g.res[0], (float)g.res[1], (float)g.res[2]};
	V3 p = V3{(float)x + 0.5f, (float)y + 0.5f, (float)z + 0.5f};
	p = add(p, d);
	p = add(p, d);
	while (p.x > 0 && p.y > 0 && p.z > 0 && p.x < s.x && p.y < s.y && p.z < s.z) {
		if (occupied(voxel_index(g, (int32_t)p.x, (int32_t)p.y, (int32_t)p.z))) return true;
		p = add(p, d);
	}
	return false;
}

// computeAO's accumulator (voxels.cpp:127-135): 1 less 1.f / ray_count once per hit, as repeated subtractions
LMX_HD float voxel_ao_of_hits(uint32_t hits, uint32_t ray_count) {
	float ao = 1;
	const float step = 1.f / (float)ray_count;
	for (uint32_t k = 0; k < hits; ++k) ao -= step;
	return ao;
}

// sample / sampleAO at a point (voxels.cpp:49-80): component-wise division, truncation; false outside [0, res)
LMX_HD bool voxel_point_cell(const VoxelGrid& g, V3 p, uint32_t* index) {
	const int32_t x = vx_i32((p.x - g.mn[0]) / (g.mx[0] - g.mn[0]) * (float)g.res[0]);
	const int32_t y = vx_i32((p.y - g.mn[1]) / (g.mx[1] - g.mn[1]) * (float)g.res[1]);
	const int32_t z = vx_i32((p.z - g.mn[2]) / (g.mx[2] - g.mn[2]) * (float)g.res[2]);
	if (x < 0 || y < 0 || z < 0 || x >= g.res[0] || y >= g.res[1] || z >= g.res[2]) return false;
	*index = voxel_index(g, x, y, z);
	return true;
}

// ModelImporter::bakeVertexAO's tail (renderer/editor/model_importer.cpp:1346)
LMX_HD uint8_t voxel_bake_u8(float ao, float min_ao) {
	const float v = (ao + min_ao) * 255;
	return (uint8_t)(vx_min(vx_max(v, 0.f), 255.f) + 0.5f);
}

#if defined(__HIPCC__)
// ---- voxel_kernels.hip -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t VOXEL_BLOCK = 256;
constexpr uint32_t VOXEL_RASTER_CELLS_PER_WAVE = 4096;  // a triangle's cell box is split over ceil(cells / this) waves, at most VOXEL_RASTER_MAX_SPLIT
constexpr uint32_t VOXEL_RASTER_MAX_SPLIT = 64;
constexpr uint32_t VOXEL_AO_LDS_WORDS = 10240;           // k_voxel_ao stages grids of up to 32 x this many cells (68^3 fits) as a bit mask in LDS; larger grids are read in global memory
constexpr uint32_t VOXEL_AO_CHUNKS_PER_WAVE = 128;       // chunks of 64 rays a wave of k_voxel_ao takes at least

enum { VOXEL_SAMPLE_VOXEL = 0, VOXEL_SAMPLE_AO = 1, VOXEL_SAMPLE_BAKE = 2 };

hipError_t launch_voxel_raster(hipStream_t s, const VoxelGrid& g, const float* tris, uint32_t n_tris, uint32_t split, uint8_t* voxels);
hipError_t launch_voxel_ao(hipStream_t s, const VoxelGrid& g, const uint8_t* voxels, uint32_t ray_count, VoxelRng seed, float* ao, bool lds); // lds: stage the mask in LDS where the grid fits
hipError_t launch_voxel_blur(hipStream_t s, const VoxelGrid& g, const float* ao, float* blurred);
// mode VOXEL_SAMPLE_VOXEL: out_u8 <- the voxel byte; _AO: out_f <- the AO; _BAKE: out_u8 <- voxel_bake_u8(AO, min_ao). inside[i] = 0 and no
// other store where the point lies outside the grid.
hipError_t launch_voxel_sample(hipStream_t s, const VoxelGrid& g, int mode, const uint8_t* voxels, const float* ao, const float* points, uint32_t n, float min_ao, uint8_t* out_u8,
	float* out_f, uint8_t* inside);
#endif

} // namespace lmx
