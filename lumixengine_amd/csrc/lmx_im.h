// lmx_im.h — device layout and launchers of the instanced-model kernels (im_kernels.hip), shared with lmx_capi_im.hip.
//
// Instances live in grid order in three dense arrays (split layout): pos_scale (float4: pos.xyz, scale), rot (float4:
// rot.xyz, 0) and lod (float). Every model's range starts on a multiple of IM_TILE, so a block's tile never straddles two models and the
// emission masks (one 64-bit word per 64 instances) line up with the waves.
#pragma once

#include "lmx_kernels.h"
#include "lumix_mi355.h"

namespace lmx {

constexpr uint32_t IM_TILE = 8192;        // instances per block of the view run (32 iterations of 256 lanes)
constexpr uint32_t IM_BLOCK = 256;
constexpr uint32_t IM_BUILD_BLOCK = 1024; // one block per model builds its grid

// One registered model as the kernels see it. Written by the host (lmx_im_set_model / set_instances / set_origins).
struct ImModelDev {
	float lod_dist[4];      // Model::getLODDistances (squared), without the multiplier
	int32_t lod_idx[4];     // running maximum of lod_indices[0..3].to (encodeInstancedModels' lod_indices.xyzw)
	float radius;           // Model::getOriginBoundingRadius
	float draw_distance;    // getDrawDistance: sqrtf of the last LOD distance whose to != -1
	uint32_t first;         // first slot of the model in the instance arrays (multiple of IM_TILE)
	uint32_t n;             // instances
	uint32_t first_tile, n_tiles; // tiles of the view run (a model without instances still owns one: it writes its counts and indirect records)
	uint32_t indirect_offset, mesh_count;
	double origin[3];       // World::getTransform(entity).pos
};

// Grid of one model: Grid::aabb, Grid::cells[16] (from relative to the model's first slot), placed / unplaced instance counts
struct ImGridDev {
	float mn[3], mx[3];
	uint32_t placed, unplaced;
	float cmin[16][3], cmax[16][3];
	uint32_t from[16], count[16];
};

// Per-view values (kernel argument)
struct ImViewDev {
	DevFrustum f;           // view.cp.frustum: the shader's u_camera_planes are f.n* / f.d (planes 0..5); getRelative also uses f.p* and f.origin
	double cam[3];
	float lod_multiplier, time_delta;
	uint32_t is_shadow, n_models;
};

// Per-model result of one run, LmxImCounts' layout
struct ImCountsDev {
	uint32_t bin_count[4], bin_offset[4];
	uint32_t indirect_offset, mesh_count, instances, unplaced;
};

struct ImArrays {
	float4* pos_scale;
	float4* rot;
	float* lod;
};

// initInstancedModelGPUData for one model: grid AABB, cells, stable scatter of `n` input records into the model's slots from `first` on.
hipError_t launch_im_grid_build(hipStream_t s, const LmxImInstance* in, uint32_t n, ImArrays a, uint32_t first, ImGridDev* grid);
// encodeInstancedModels for every model in two launches: k_im_count (cell verdicts, LOD update, sphere test, per-tile bin counts, emission
// masks, the models' bin totals) and k_im_emit (bin offsets, indirect records, per-model counts, ordered compaction). tile_model: the model of
// each tile. model_tot: 4 words per model, zero on entry (k_im_count adds into it); model_tot_next: the other half of that double buffer,
// cleared by k_im_emit for the next run.
hipError_t launch_im_run(hipStream_t s, const ImModelDev* models, const ImGridDev* grids, const uint32_t* tile_model, uint32_t n_tiles, const ImViewDev& view,
	ImArrays a, const uint32_t* indices_count, uint64_t* masks, uint4* tile_counts, uint32_t* model_tot, uint32_t* model_tot_next, LmxImInstance* records,
	LmxImIndirect* indirect, ImCountsDev* counts);


// What the ray casts read of an instanced-models object (lmx_capi_rays.hip): its context, and its tables as they are now - uploaded first
// if a set_* call changed them (that waits for the stream).
struct ImRayTables {
	const ImModelDev* models; uint32_t n_models;
	const uint32_t* tile_model; uint32_t n_tiles;
	const float4* pos_scale; const float4* rot;
};
LmxContext* im_context(const LmxInstancedModels* im);
uint32_t im_model_count(const LmxInstancedModels* im);
int im_ray_tables(LmxInstancedModels* im, ImRayTables* out);

} // namespace lmx
