// gpu_cluster_filler.h — the fillClusters stand-in (C++ host side of include/lumix_mi355.h "clustered lights and probes").
//
// In the reference PipelineImpl::fillClusters (src/renderer/pipeline.cpp:3327-3684) asks the culling system for the view's visible
// LOCAL_LIGHT entities, turns them into ClusterLight records, bins lights, environment probes and reflection probes into the view's
// cluster grid on one thread and uploads `lights`, `clusters`, `cluster_map`, `env_probes` and `refl_probes`. GpuClusterFiller does the
// same behind lmx_cull without the list ever reaching the host: the tables go up when lights / probes change, fill() enqueues the pass
// over the cull result in a view slot, deviceOutputs() names the five buffers to bind. The shadow atlas (:3384-3442) stays with the
// engine: setAtlas() carries its entity -> slot map.
//
// `Module` is RenderModule inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any type with its light / probe
// getters (tests/cpp/lumix_compat_lights.h).
#pragma once

#include <cstring>
#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/geometry.h"
	#include "core/math.h"
	#include "renderer/render_module.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_lights.h"
#endif

namespace Lumix {

static_assert(sizeof(ShiftedFrustum) == sizeof(LmxShiftedFrustum), "ShiftedFrustum is 256 bytes");
// the environment probes go to the library as they are
static_assert(sizeof(EnvironmentProbe) == sizeof(LmxEnvProbe), "EnvironmentProbe is 136 bytes");
static_assert(offsetof(EnvironmentProbe, outer_range) == offsetof(LmxEnvProbe, outer_range), "EnvironmentProbe::outer_range");
static_assert(offsetof(EnvironmentProbe, flags) == offsetof(LmxEnvProbe, flags), "EnvironmentProbe::flags");
static_assert(offsetof(EnvironmentProbe, sh_coefs) == offsetof(LmxEnvProbe, sh_coefs), "EnvironmentProbe::sh_coefs");
static_assert((u32)EnvironmentProbe::ENABLED == (u32)LMX_PROBE_ENABLED && (u32)ReflectionProbe::ENABLED == (u32)LMX_PROBE_ENABLED, "the ENABLED flag");

struct GpuClusterFiller {
	explicit GpuClusterFiller(LmxContext* ctx) : m_ctx(ctx) {}

	// Every PointLight of the module by entity index; n_entities = the entity range of the transform tables. Call when lights change.
	template <typename Module> bool setLights(Module& module, u32 n_entities) {
		m_lights.assign(n_entities, LmxPointLight{});
		for (const PointLight& pl : module.getPointLights()) {
			const i32 e = pl.entity.index;
			if (e < 0 || (u32)e >= n_entities) continue;
			LmxPointLight& out = m_lights[e];
			out.color[0] = pl.color.x; out.color[1] = pl.color.y; out.color[2] = pl.color.z;
			out.intensity = pl.intensity;
			out.range = pl.range;
			out.fov = pl.fov;
			out.attenuation_param = pl.attenuation_param;
			out.flags = (uint32_t)pl.flags;
		}
		return lmx_clusters_set_lights(m_ctx, n_entities, m_lights.data()) == LMX_OK;
	}

	// The module's environment and reflection probes with their entities, module order. Call when probes change (or are enabled / disabled).
	template <typename Module> bool setProbes(Module& module) {
		const Span<const EnvironmentProbe> env = module.getEnvironmentProbes();
		const Span<const ReflectionProbe> refl = module.getReflectionProbes();
		const Span<EntityRef> env_entities = module.getEnvironmentProbesEntities();
		const Span<EntityRef> refl_entities = module.getReflectionProbesEntities();
		std::vector<int32_t> ee(env.length()), re(refl.length());
		std::vector<LmxReflProbe> rp(refl.length());
		for (u32 i = 0; i < env.length(); ++i) ee[i] = env_entities[i].index;
		for (u32 i = 0; i < refl.length(); ++i) {
			re[i] = refl_entities[i].index;
			rp[i].half_extents[0] = refl[i].half_extents.x; rp[i].half_extents[1] = refl[i].half_extents.y; rp[i].half_extents[2] = refl[i].half_extents.z;
			rp[i].texture_id = refl[i].texture_id;
			rp[i].flags = (uint32_t)refl[i].flags;
		}
		return lmx_clusters_set_probes(m_ctx, env.length(), reinterpret_cast<const LmxEnvProbe*>(env.begin()), ee.data(), refl.length(), rp.data(), re.data()) == LMX_OK;
	}

	// m_shadow_atlas.map as a table by entity index (0xffffffff: no slot); nullptr: no light has one
	bool setAtlas(const uint32_t* atlas_idx, u32 n_entities) { return lmx_clusters_set_atlas(m_ctx, n_entities, atlas_idx) == LMX_OK; }

	bool reserve(u32 max_lights, u32 map_capacity) { return lmx_clusters_reserve(m_ctx, max_lights, map_capacity) == LMX_OK; }

	// Behind the cull of the view's light query into `view_slot` (lmx_cull with LOCAL_LIGHT or all types). Enqueues and returns.
	bool fill(u32 view_slot, const ShiftedFrustum& frustum, const DVec3& cam_pos, u32 w, u32 h) {
		LmxClusterView cv;
		memset(&cv, 0, sizeof(cv));
		cv.camera_pos[0] = cam_pos.x; cv.camera_pos[1] = cam_pos.y; cv.camera_pos[2] = cam_pos.z;
		memcpy(&cv.frustum, &frustum, sizeof(cv.frustum));
		cv.viewport_w = w;
		cv.viewport_h = h;
		return lmx_clusters_run(m_ctx, view_slot, 0, &cv) == LMX_OK;
	}

	// {lights, env_probes, refl_probes, map_entries, overflow} of the last fill (synchronizes); an overflow bit asks for a larger reserve()
	bool counts(LmxClustersCounts& out) { return lmx_clusters_counts(m_ctx, &out) == LMX_OK; }

	// the five shader buffers in HBM and the counters, stream-ordered behind fill()
	bool deviceOutputs(LmxClustersDevice& out) { return lmx_clusters_device_outputs(m_ctx, &out) == LMX_OK; }

	const char* lastError() const { return lmx_last_error(m_ctx); }

private:
	LmxContext* m_ctx;
	std::vector<LmxPointLight> m_lights;
};

} // namespace Lumix
