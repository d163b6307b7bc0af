// voxels_host_sanitize.cpp — the host-side arithmetic of csrc/lmx_voxels.h (grid, cell boxes, the box/triangle test, the generator's skip,
// the march, the lookups, the bake) at its edges, as a stand-alone program: tests/test_voxels_cpu.py builds it with
// -fsanitize=address,undefined and expects it to run clean. Inputs are what the C ABI lets through and what it refuses on the way in.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lmx_voxels.h"

using namespace lmx;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	// the conversions: every float, finite or not, has a defined result
	const float edge[] = {0.f, -0.f, 0.5f, -0.3f, 2147483520.f, 2147483648.f, -2147483648.f, -2147483904.f, 3e38f, -3e38f, inf, -inf, nan, FLT_MIN, -FLT_MIN};
	for (float v : edge) (void)vx_i32(v);
	CHECK(vx_i32(-0.3f) == 0 && vx_i32(2147483648.f) == INT32_MIN && vx_i32(nan) == INT32_MIN && vx_i32(-2147483648.f) == INT32_MIN && vx_i32(2147483520.f) == 2147483520);
	// grids of boxes the entry points refuse only after computing them
	for (float a : edge)
		for (float b : edge)
			for (uint32_t res : {1u, 4u, 64u, 0xffffffffu}) {
				const float mn[3] = {a, 0.f, b}, mx[3] = {b, 1.f, a};
				const VoxelGrid g = voxel_grid(mn, mx, res);
				(void)g;
			}
	const float mn[3] = {0, 0, 0}, mx[3] = {1, 1, 1};
	const VoxelGrid g = voxel_grid(mn, mx, 4);
	CHECK(g.res[0] == 7 && g.res[1] == 7 && g.res[2] == 7 && voxel_cells(g) == 343);
	// cell boxes of triangles far outside, larger than the grid, degenerate, at the float range's end
	std::vector<uint8_t> voxels(voxel_cells(g), 0);
	const V3 pts[] = {{0.2f, 0.2f, 0.2f}, {0.9f, 0.1f, 0.5f}, {-3e38f, 3e38f, 0.f}, {3e38f, 3e38f, 3e38f}, {1e9f, -1e9f, 1e9f}, {0.5f, 0.5f, 0.5f}, {-40.f, -40.f, 0.4f}, {40.f, -40.f, 0.4f}, {0.f, 60.f, 0.4f}};
	const size_t n_pts = sizeof(pts) / sizeof(pts[0]);
	for (size_t a = 0; a < n_pts; ++a)
		for (size_t b = 0; b < n_pts; ++b)
			for (size_t c = 0; c < n_pts; ++c) {
				const VoxelSpan s = voxel_clip_box(g, voxel_triangle_box(g, pts[a], pts[b], pts[c]));
				CHECK(s.n <= voxel_cells(g));
				for (uint64_t cell = 0; cell < s.n; ++cell) {
					const uint32_t cc = (uint32_t)cell, ci = cc % s.ext[0], rest = cc / s.ext[0];
					const int32_t i = s.lo[0] + (int32_t)ci, j = s.lo[1] + (int32_t)(rest % s.ext[1]), k = s.lo[2] + (int32_t)(rest / s.ext[1]);
					CHECK(i >= 0 && j >= 0 && k >= 0 && i < g.res[0] && j < g.res[1] && k < g.res[2]);
					if (voxel_cell_hits_triangle(g, i, j, k, pts[a], pts[b], pts[c])) voxels[voxel_index(g, i, j, k)] = 1;
				}
			}
	// the generator: the skip against sequential stepping, edge seeds, and composition over long jumps
	const uint32_t seeds[] = {1u, 0xffffffffu, 0x80000000u, (uint32_t)VOXEL_RNG_M_U, (uint32_t)VOXEL_RNG_M_U + 1u, (uint32_t)VOXEL_RNG_M_V - 1u, (uint32_t)VOXEL_RNG_M_V, 65535u, 65536u, 0u};
	for (uint32_t su : seeds)
		for (uint32_t sv : seeds) {
			VoxelRng seq = {su, sv};
			for (uint64_t n = 0; n <= 200; ++n) {
				const VoxelRng jump = voxel_rng_skip(VoxelRng{su, sv}, n);
				CHECK(jump.u == seq.u && jump.v == seq.v);
				(void)seq.rand();
			}
			const VoxelRng a = voxel_rng_skip(voxel_rng_skip(VoxelRng{su, sv}, 1000003ull), 0xfffffffffffull), b = voxel_rng_skip(VoxelRng{su, sv}, 1000003ull + 0xfffffffffffull);
			CHECK(a.u == b.u && a.v == b.v);
			(void)voxel_rng_skip(VoxelRng{su, sv}, ~0ull);
		}
	// rays: every direction the draws can give, NaN included, stays inside the grid's bytes
	VoxelRng rng = {1824158168u, 1797839u};
	uint32_t hits = 0;
	for (int32_t z = 0; z < g.res[2]; ++z)
		for (int32_t y = 0; y < g.res[1]; ++y)
			for (int32_t x = 0; x < g.res[0]; ++x)
				for (int d = 0; d < 8; ++d) {
					const V3 dir = voxel_ray_dir(rng);
					hits += voxel_cast_ray(g, x, y, z, dir, [&](uint32_t idx) { CHECK(idx < voxels.size()); return voxels[idx < voxels.size() ? idx : 0]; }) ? 1u : 0u;
				}
	for (V3 dir : {V3{nan, nan, nan}, V3{inf, -inf, 1}, V3{1e-30f, 1, -1e-30f}}) // (a direction's largest component is +-1 or NaN: voxel_ray_dir)
		(void)voxel_cast_ray(g, 3, 3, 3, dir, [&](uint32_t idx) { CHECK(idx < voxels.size()); return 0; });
	CHECK(hits > 0);
	CHECK(voxel_ao_of_hits(0, 5) == 1.f && voxel_ao_of_hits(5, 5) != voxel_ao_of_hits(4, 5));
	// lookups and the bake for any point and any AO
	for (float a : edge)
		for (float b : edge) {
			uint32_t idx = 0;
			if (voxel_point_cell(g, V3{a, b, 0.5f}, &idx)) CHECK(idx < voxels.size());
			(void)voxel_bake_u8(a, b);
		}
	CHECK(voxel_bake_u8(1.f, 0.3f) == 255 && voxel_bake_u8(0.f, 0.f) == 0 && voxel_bake_u8(nan, 0.f) == 0 && voxel_bake_u8(0.5f, 0.f) == 128);
	printf(failures ? "voxels host arithmetic: %d checks failed\n" : "voxels host arithmetic: clean\n", failures);
	return failures ? 1 : 0;
}
