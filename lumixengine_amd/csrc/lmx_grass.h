// lmx_grass.h — device layouts and launchers of grass_kernels.hip (Terrain::createGrass's quads, renderGrass's quad loop), shared with
// lmx_capi_grass.hip. Nothing here crosses the C ABI.
#pragma once

#include "lmx_kernels.h"

namespace lmx {

constexpr uint32_t GRASS_BLOCK = 64;        // k_grass_quads: one wave per quad
constexpr uint32_t GRASS_WINDOW = 64;       // texels per side of the splat window a block stages in LDS; a larger window reads global memory
constexpr uint32_t GRASS_CULL_BLOCK = 256;  // k_grass_cull: one block per view walks the live list in tiles of this many quads
static_assert(GRASS_BLOCK == 64 && GRASS_CULL_BLOCK % 64 == 0, "whole waves");
static_assert(LMX_GRASS_SLOT_INSTANCES == 2 * LMX_GRASS_SAMPLES, "every accepted sample is stored twice");

struct GrassTerrainDev {
	uint64_t height_at, splat_at;  // bytes into the texel buffer, 4-byte aligned
	uint32_t width, height, format; // the heightmap (LMX_RAY_TERRAIN_*)
	float scale[3];
	uint32_t splat_w, splat_h;
	uint32_t splat_ok;             // RGBA8 with data: anything else gives 0 for every texel
	uint32_t pad;
};
struct GrassJob { uint32_t terrain, type, i, j, slot, rotation_mode; float spacing; uint32_t pad; }; // a quad createGrass creates
struct GrassGroupDev { uint32_t terrain, type; float spacing, distance; uint32_t usable, pad; };     // a (terrain, grass type)
struct GrassLive { uint32_t slot, group; };                                                           // a cached quad, in (terrain, type, i, j) order
struct GrassViewDev { DevFrustum f; double viewport[3]; float lod_multiplier; uint32_t pad; };

struct GrassQuadsDevice {
	const GrassTerrainDev* terrains;
	const uint8_t* texels;
	const GrassJob* jobs;
	uint32_t n_jobs;
	float4* pool;            // slot s: 2 float4 per record, LMX_GRASS_SLOT_INSTANCES records
	LmxGrassQuad* quads;     // by slot
};
struct GrassCullDevice {
	const GrassViewDev* views;
	const GrassLive* live;
	uint32_t n_live, draw_stride;
	const GrassGroupDev* groups;
	const double* terrain_pos; // 3 per terrain
	const LmxGrassQuad* quads;
	LmxGrassDraw* draws;       // [view][draw_stride]
	LmxGrassCounts* counts;    // [view]
};

hipError_t launch_grass_quads(hipStream_t s, const GrassQuadsDevice& d);                  // one block per job
hipError_t launch_grass_cull(hipStream_t s, const GrassCullDevice& d, uint32_t n_views);  // one block per view

} // namespace lmx
