// gpu_grass.h — the Terrain::createGrass / renderGrass quad-loop stand-in (C++ host side of include/lumix_mi355.h "Terrain grass").
//
// In the reference PipelineImpl::renderGrass (src/renderer/pipeline.cpp:2106-2210) calls Terrain::createGrass(center, frame) for every
// terrain on the thread that starts the frame and pushes a job that, per terrain, per grass type, per mesh of LOD 0, walks the type's
// quads: frustum test, distance, instance count, one drawIndexedInstanced. GpuGrass keeps those two steps over lmx_grass_*:
//   setTerrains(terrains)      when a terrain, its maps or its grass types change (Terrain::setGrassDirty: invalidate(index))
//   createGrass(cp_pos, frame) center = -(tr.pos - cp.pos).xz per terrain, as renderGrass computes it (:2110-2113); false = the pool is
//                              short or an argument is out of range: the engine runs its own createGrass / renderGrass this frame
//   cull(views, n)             every view of the frame in one launch
//   getDraws(out)              the device pointers renderGrass's job binds: per view d_counts[v].draws records {slot, instance_count,
//                              distance, terrain, type} at d_draws + v * draw_stride; the quad's instances are the slice
//                              d_pool + slot * LMX_GRASS_SLOT_INSTANCES. The job replays a view's records once per mesh of LOD 0.
// Programs, materials, uniform pools and the draw stream stay with the engine's job. Nothing here waits for the device.
//
// `TerrainT` is Terrain inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any type with m_heightmap, m_splatmap,
// m_scale, m_width, m_height, m_entity and m_grass_types (tests/cpp/lumix_compat_grass.h).
#pragma once

#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/geometry.h"
	#include "core/math.h"
	#include "engine/world.h"
	#include "renderer/gpu/gpu.h"
	#include "renderer/model.h"
	#include "renderer/terrain.h"
	#include "renderer/texture.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_grass.h"
#endif

namespace Lumix {

static_assert(sizeof(ShiftedFrustum) == sizeof(LmxShiftedFrustum), "ShiftedFrustum is 256 bytes");

struct GpuGrass {
	// a view of renderGrass: cp.frustum, the pipeline's m_viewport.pos (also for shadow views), Renderer::getLODMultiplier()
	struct View {
		const ShiftedFrustum* frustum;
		DVec3 viewport_pos;
		float lod_multiplier;
	};

	explicit GpuGrass(LmxContext* ctx, u32 slots) : m_ctx(ctx) {
		lmx_grass_create(ctx, &m_grass);
		lmx_grass_reserve(m_grass, slots);
	}
	~GpuGrass() { lmx_grass_destroy(m_grass); }
	GpuGrass(const GpuGrass&) = delete;
	void operator=(const GpuGrass&) = delete;

	// RenderModule::getTerrains() in the order the engine keeps: index k here is `terrain` of every record. Drops every cached quad.
	template <typename TerrainT> bool setTerrains(TerrainT* const* terrains, u32 n) {
		std::vector<LmxGrassTerrain> recs(n);
		std::vector<std::vector<LmxGrassType>> types(n);
		m_entities.resize(n);
		for (u32 k = 0; k < n; ++k) {
			const TerrainT& t = *terrains[k];
			LmxGrassTerrain& r = recs[k];
			r = {};
			m_entities[k] = t.m_entity.index;
			r.heightmap.entity = t.m_entity.index;
			r.heightmap.width = (u32)t.m_width; r.heightmap.height = (u32)t.m_height;
			r.heightmap.scale[0] = t.m_scale.x; r.heightmap.scale[1] = t.m_scale.y; r.heightmap.scale[2] = t.m_scale.z;
			r.heightmap.format = LMX_RAY_TERRAIN_R16;
			if (t.m_heightmap && t.m_heightmap->isReady() && t.m_heightmap->getData()
				&& (t.m_heightmap->format == gpu::TextureFormat::R16 || t.m_heightmap->format == gpu::TextureFormat::RGBA8)) {
				r.heightmap.format = t.m_heightmap->format == gpu::TextureFormat::R16 ? LMX_RAY_TERRAIN_R16 : LMX_RAY_TERRAIN_RGBA8;
				r.heightmap.ready = 1;
				r.heightmap.texels = t.m_heightmap->getData();
			}
			if (t.m_splatmap) {
				r.splat_ready = t.m_splatmap->isReady() ? 1 : 0;
				r.splat_width = t.m_splatmap->width; r.splat_height = t.m_splatmap->height;
				r.splat_format = t.m_splatmap->format == gpu::TextureFormat::RGBA8 ? LMX_RAY_TERRAIN_RGBA8 : ~0u;
				r.splat_texels = t.m_splatmap->getData();
			}
			for (const auto& type : t.m_grass_types) {
				LmxGrassType ty;
				ty.spacing = type.m_spacing; ty.distance = type.m_distance;
				ty.rotation_mode = type.m_rotation_mode == GrassRotationMode::ALL_RANDOM ? LMX_GRASS_ROTATION_ALL_RANDOM : LMX_GRASS_ROTATION_Y_UP;
				ty.usable = type.m_grass_model && type.m_grass_model->isReady() ? 1 : 0;
				types[k].push_back(ty);
			}
			r.types = types[k].data();
			r.n_types = (u32)types[k].size();
		}
		m_positions.assign(3 * (size_t)n, 0.0);
		m_centers.assign(2 * (size_t)n, 0.f);
		return lmx_grass_set_terrains(m_grass, n, recs.data()) == LMX_OK;
	}

	bool invalidate(u32 terrain) { return lmx_grass_invalidate(m_grass, terrain) == LMX_OK; } // Terrain::setGrassDirty

	// renderGrass's first loop (:2109-2114) for every terrain: World::getPosition of the entity, the centre, createGrass
	template <typename WorldT> bool createGrass(const WorldT& world, const DVec3& cp_pos, u32 frame) {
		const u32 n = (u32)m_entities.size();
		for (u32 k = 0; k < n; ++k) {
			const DVec3 pos = world.getPosition(EntityRef{m_entities[k]});
			m_positions[3 * (size_t)k] = pos.x; m_positions[3 * (size_t)k + 1] = pos.y; m_positions[3 * (size_t)k + 2] = pos.z;
			m_centers[2 * (size_t)k] = -(float)(pos.x - cp_pos.x); // Vec2(-(float)rel_tr.pos.x, -(float)rel_tr.pos.z)
			m_centers[2 * (size_t)k + 1] = -(float)(pos.z - cp_pos.z);
		}
		if (lmx_grass_set_positions(m_grass, n, m_positions.data()) != LMX_OK) return false;
		return lmx_grass_update(m_grass, frame, n, m_centers.data()) == LMX_OK;
	}

	bool cull(const View* views, u32 n) {
		m_views.resize(n);
		for (u32 v = 0; v < n; ++v) {
			m_views[v] = {};
			m_views[v].frustum = reinterpret_cast<const LmxShiftedFrustum&>(*views[v].frustum);
			m_views[v].viewport_pos[0] = views[v].viewport_pos.x; m_views[v].viewport_pos[1] = views[v].viewport_pos.y; m_views[v].viewport_pos[2] = views[v].viewport_pos.z;
			m_views[v].lod_multiplier = views[v].lod_multiplier;
		}
		return lmx_grass_cull(m_grass, n, m_views.data()) == LMX_OK;
	}

	// what the job binds: the pool, the quad records, the draws and counts of the last cull (device pointers, stream-ordered)
	bool getDraws(LmxGrassDevice& out) const { return lmx_grass_device_outputs(m_grass, &out) == LMX_OK; }

	const char* lastError() const { return lmx_last_error(m_ctx); }
	LmxGrass* handle() const { return m_grass; }

private:
	LmxContext* m_ctx;
	LmxGrass* m_grass = nullptr;
	std::vector<i32> m_entities;
	std::vector<double> m_positions;
	std::vector<float> m_centers;
	std::vector<LmxGrassView> m_views;
};

} // namespace Lumix
