// gpu_ray_caster.h — the castRay stand-in (C++ host side of include/lumix_mi355.h "ray casts").
//
// In the reference RenderModuleImpl::castRay (src/renderer/render_module.cpp:2715-2780) walks every model instance on one thread and every
// LOD-0 triangle of the instances its gates let through. GpuRayCaster answers a batch of rays where the transforms, palettes and meshes
// already lie: castRays() uploads the rays, enqueues the cast and reads one record per ray back. What the device does not hold -
// general filter delegates, and procedural geometry and terrain until their tables are set - stays with the caller: it casts those first, passes the best hit it
// holds as `held` (its t becomes the ray's t_max, so farther model instances are pruned as the reference's walk prunes them), and gets
// the nearer of the two back, compared as :2746 and :2761-2775 compare them. Only the filter of castRay(ray, ignored) is supported.
//
// Instanced models (castRayInstancedModels, :2609-2648, the first thing castRay does) are cast on the device too once the
// gpu_instanced_models.h adapter is attached with setInstancedModels(): the hit comes back with component_type = types::instanced_model,
// the model's entity, subindex, mesh and t wherever no model instance is strictly nearer, and `held` shrinks to procedural geometry and
// terrain. Without an attached adapter they stay with the caller as before.
//
// Procedural geometry (castRayProceduralGeometry, :2650-2712) and terrains (Terrain::castRay, terrain.cpp:474-535) are cast on the device as
// well once setProceduralGeometries(module) / setTerrains(module) have filled their tables: castRays() then takes the whole result of
// castRay(ray, ignored) - the merge of :2761-2775 included - from one LmxRaySceneHit per ray, with component_type = the procedural_geom or
// terrain type of setSceneTypes(), mesh = nullptr and the entity of :2703 / :2771, and `held` shrinks to what general filter delegates
// leave with the caller. Call them again when a geometry or a heightmap changes.
//
// The geometry tables go up through the C ABI when models load (lmx_rays_add_mesh / lmx_rays_set_models / lmx_rays_set_instances: an
// engine has the vertex and index arrays at hand in Model::onBeforeReady); transforms come from where the draw pass takes them.
//
// `Module` is RenderModule inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any type with getModelInstances()
// (tests/cpp/lumix_compat.h + lumix_compat_rays.h).
#pragma once

#include <cmath>
#include <vector>

#include "lumix_mi355.h"
#include "gpu_instanced_models.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/geometry.h"
	#include "core/math.h"
	#include "renderer/gpu/gpu.h"
	#include "renderer/model.h"
	#include "renderer/render_module.h"
	#include "renderer/terrain.h"
	#include "renderer/texture.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_rays.h"
	#include "lumix_compat_scene_rays.h"
#endif

namespace Lumix {

struct GpuRayCaster {
	// model_instance_type: the component type the hits carry (types::model_instance of the renderer)
	GpuRayCaster(LmxContext* ctx, ComponentType model_instance_type) : m_ctx(ctx), m_type(model_instance_type) {}

	// Attach the instanced models (nullptr: detach). Per slot of `im`, in its registration order: ray_model = the model's id in
	// lmx_rays_set_models (-1: it has no Model, or is not cast), models = the engine's Model (RayCastModelHit::mesh points into it).
	// Call again when a model is registered with `im`. instanced_model_type: types::instanced_model of the renderer.
	bool setInstancedModels(GpuInstancedModels* im, ComponentType instanced_model_type, const i32* ray_model, Model* const* models) {
		m_im = nullptr;
		m_im_models.clear();
		if (!im) return lmx_rays_set_instanced_models(m_ctx, nullptr, 0, nullptr, nullptr) == LMX_OK;
		const std::vector<int32_t>& entities = im->entities();
		const u32 n = (u32)entities.size();
		if (lmx_rays_set_instanced_models(m_ctx, im->handle(), n, ray_model, entities.data()) != LMX_OK) return false;
		m_im_models.assign(models, models + n);
		m_im_type = instanced_model_type;
		m_im = im;
		return true;
	}

	// The component types the procedural-geometry and terrain hits carry (types::procedural_geom, types::terrain of the renderer)
	void setSceneTypes(ComponentType procedural_geom_type, ComponentType terrain_type) {
		m_pg_type = procedural_geom_type;
		m_terrain_type = terrain_type;
	}

	// RenderModule::getProceduralGeometries() in its iterated() order -> the device's table (an empty map clears it). The vertex and index
	// streams are copied before the call returns.
	template <typename Module> bool setProceduralGeometries(Module& module) {
		std::vector<LmxRayProcGeom> recs;
		const auto& geometries = module.getProceduralGeometries(); // (const: walked through begin() / end(), the order of iterated())
		for (auto iter = geometries.begin(), end = geometries.end(); iter != end; ++iter) {
			const ProceduralGeometry& pg = iter.value();
			LmxRayProcGeom g = {};
			g.entity = iter.key().index;
			g.triangles = pg.vertex_decl.primitive_type == gpu::PrimitiveType::TRIANGLES ? 1u : 0u;
			g.aabb_min[0] = pg.aabb.min.x; g.aabb_min[1] = pg.aabb.min.y; g.aabb_min[2] = pg.aabb.min.z;
			g.aabb_max[0] = pg.aabb.max.x; g.aabb_max[1] = pg.aabb.max.y; g.aabb_max[2] = pg.aabb.max.z;
			g.vertex_data = pg.vertex_data.data();
			g.vertex_bytes = (u32)pg.vertex_data.size();
			g.stride = pg.vertex_decl.getStride();
			g.index_data = pg.index_data.data();
			g.index_bytes = pg.index_data.size() == 0 ? 0u : (pg.index_type == gpu::DataType::U16 ? 2u : 4u);
			g.index_count = pg.getIndexCount();
			recs.push_back(g);
		}
		if (lmx_rays_set_procedural_geometries(m_ctx, (u32)recs.size(), recs.data()) != LMX_OK) return false; // (the device keeps the table it had)
		m_n_pg = (u32)recs.size();
		return true;
	}

	// RenderModule::getTerrains() in its own order (the merge is sequential) -> the device's table. A terrain whose heightmap is missing,
	// not ready, without data or in a format Terrain::getHeight does not read is kept in the table and never hit.
	template <typename Module> bool setTerrains(Module& module) {
		std::vector<LmxRayTerrain> recs;
		for (Terrain* terrain : module.getTerrains()) {
			const Texture* hm = terrain->getHeightmap();
			LmxRayTerrain t = {};
			t.entity = terrain->getEntity().index;
			t.width = (u32)terrain->getWidth();
			t.height = (u32)terrain->getHeight();
			const Vec3 scale = terrain->getScale();
			t.scale[0] = scale.x; t.scale[1] = scale.y; t.scale[2] = scale.z;
			const bool known = hm && (hm->format == gpu::TextureFormat::R16 || hm->format == gpu::TextureFormat::RGBA8);
			t.format = known && hm->format == gpu::TextureFormat::RGBA8 ? LMX_RAY_TERRAIN_RGBA8 : LMX_RAY_TERRAIN_R16;
			t.texels = hm ? hm->getData() : nullptr;
			t.ready = known && hm->isReady() && t.texels && t.width && t.height ? 1u : 0u;
			recs.push_back(t);
		}
		if (lmx_rays_set_terrains(m_ctx, (u32)recs.size(), recs.data()) != LMX_OK) return false; // (the device keeps the table it had)
		m_n_terrains = (u32)recs.size();
		return true;
	}

	bool reserve(u32 max_rays, u32 max_candidates) { return lmx_rays_reserve(m_ctx, max_rays, max_candidates) == LMX_OK; }

	// RenderModule::castRay(ray, ignored) over the model instances. held: the nearest hit of what the device does not cast, or nullptr.
	template <typename Module> RayCastModelHit castRay(Module& module, const Ray& ray, EntityPtr ignored, const RayCastModelHit* held = nullptr) {
		RayCastModelHit hit;
		castRays(module, Span<const Ray>(&ray, 1), Span<RayCastModelHit>(&hit, 1), ignored, held);
		return hit;
	}

	// One hit per ray: origin, dir, entity, mesh, component_type and t as the reference fills them; is_hit = false where nothing is met.
	// held (optional, one per ray): see above. False when the cast failed or the candidate list overflowed (counts() names the size needed).
	template <typename Module> bool castRays(Module& module, Span<const Ray> rays, Span<RayCastModelHit> hits, EntityPtr ignored, const RayCastModelHit* held = nullptr) {
		const u32 n = rays.length();
		if (hits.length() < n) return false;
		m_rays.resize(n);
		m_hits.resize(n);
		for (u32 i = 0; i < n; ++i) {
			LmxRay& r = m_rays[i];
			r.origin[0] = rays[i].origin.x; r.origin[1] = rays[i].origin.y; r.origin[2] = rays[i].origin.z;
			r.dir[0] = rays[i].dir.x; r.dir[1] = rays[i].dir.y; r.dir[2] = rays[i].dir.z;
			r.t_max = held && held[i].is_hit ? held[i].t : INFINITY;
			r.ignore = ignored.isValid() ? ignored.index : -1;
			r._pad = 0;
		}
		if (m_im && !m_im->flushOrigins()) return false;
		if (lmx_rays_cast(m_ctx, m_rays.data(), n) != LMX_OK) return false;
		LmxRaysCounts c;
		if (lmx_rays_counts(m_ctx, &c) != LMX_OK || c.overflow) return false; // (bit 1: the instanced-model stage, bit 2: the procedural geometries)
		if (lmx_rays_read_hits(m_ctx, m_hits.data(), n) != LMX_OK) return false;
		m_im_hits.resize(m_im ? n : 0);
		if (m_im && lmx_rays_read_im_hits(m_ctx, m_im_hits.data(), n) != LMX_OK) return false;
		const bool scene = m_n_pg != 0 || m_n_terrains != 0; // the device merged all four stages (:2761-2775)
		m_scene_hits.resize(scene ? n : 0);
		if (scene && lmx_rays_read_scene_hits(m_ctx, m_scene_hits.data(), n) != LMX_OK) return false;
		auto instances = module.getModelInstances();
		for (u32 i = 0; i < n; ++i) {
			RayCastModelHit& out = hits[i];
			const LmxRayHit& h = m_hits[i];
			if (scene && m_scene_hits[i].is_hit && (m_scene_hits[i].component == LMX_RAY_HIT_PROCEDURAL_GEOM || m_scene_hits[i].component == LMX_RAY_HIT_TERRAIN)) {
				const LmxRaySceneHit& s = m_scene_hits[i]; // nearer than the model-instance and instanced-model hits as :2762 / :2769 compare them
				out.is_hit = true;
				out.t = s.t;
				out.entity = EntityPtr{s.entity}; // iter.key() (:2703) / terrain->getEntity() (:2771)
				out.component_type = s.component == LMX_RAY_HIT_TERRAIN ? m_terrain_type : m_pg_type;
				out.subindex = 0;
				out.mesh = nullptr;
			}
			// `!hit.is_hit || new_t < hit.t` (:2746) was applied on the device through t_max: a device hit is the nearer one
			else if (h.is_hit) {
				out.is_hit = true;
				out.t = h.t;
				out.entity = EntityPtr{h.entity};
				out.component_type = m_type;
				out.subindex = 0;
				const auto* model = (u32)h.entity < instances.length() ? instances[h.entity].model : nullptr;
				out.mesh = model ? const_cast<Mesh*>(&model->getMesh(h.mesh)) : nullptr;
			} else if (m_im && m_im_hits[i].is_hit) { // below t_max, so nearer than `held`; no model instance is strictly nearer (:2746)
				const LmxRayImHit& ih = m_im_hits[i];
				out.is_hit = true;
				out.t = ih.t;
				out.entity = EntityPtr{ih.entity};
				out.component_type = m_im_type;
				out.subindex = ih.subindex;
				Model* model = ih.model < m_im_models.size() ? m_im_models[ih.model] : nullptr;
				out.mesh = model ? const_cast<Mesh*>(&model->getMesh(ih.mesh)) : nullptr;
			} else if (held && held[i].is_hit) {
				out = held[i];
			} else {
				out.is_hit = false;
				out.t = 0;
				out.mesh = nullptr;
				out.entity = EntityPtr{-1};
				out.subindex = 0;
			}
			out.origin = rays[i].origin; // :2777-2778
			out.dir = rays[i].dir;
		}
		return true;
	}

	// The merge of :2761-2775 for a hit found behind the device cast (procedural geometry, a terrain): it replaces `hit` when it is nearer.
	static void merge(RayCastModelHit& hit, const RayCastModelHit& other) {
		if (other.is_hit && (!hit.is_hit || other.t < hit.t)) {
			const DVec3 origin = hit.origin;
			const Vec3 dir = hit.dir;
			hit = other;
			hit.origin = origin;
			hit.dir = dir;
		}
	}

	bool counts(LmxRaysCounts& out) { return lmx_rays_counts(m_ctx, &out) == LMX_OK; }
	bool imCounts(LmxRaysImCounts& out) { return lmx_rays_im_counts(m_ctx, &out) == LMX_OK; }
	bool sceneCounts(LmxRaysSceneCounts& out) { return lmx_rays_scene_counts(m_ctx, &out) == LMX_OK; }
	const char* lastError() const { return lmx_last_error(m_ctx); }

private:
	LmxContext* m_ctx;
	ComponentType m_type;
	std::vector<LmxRay> m_rays;
	std::vector<LmxRayHit> m_hits;
	GpuInstancedModels* m_im = nullptr;
	ComponentType m_im_type = {};
	std::vector<Model*> m_im_models;
	std::vector<LmxRayImHit> m_im_hits;
	ComponentType m_pg_type = {};
	ComponentType m_terrain_type = {};
	u32 m_n_pg = 0, m_n_terrains = 0;
	std::vector<LmxRaySceneHit> m_scene_hits;
};

} // namespace Lumix
