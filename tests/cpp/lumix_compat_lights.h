// lumix_compat_lights.h — what gpu_cluster_filler.h reads of the renderer's lights and probes, for STANDALONE builds (TEST INFRASTRUCTURE,
// beside lumix_compat.h): the public shape of
//   PointLight / ReflectionProbe / EnvironmentProbe     src/renderer/render_module.h:156-203
//   RenderModule::getPointLights, getEnvironmentProbes(Entities), getReflectionProbes(Entities)   src/renderer/render_module.h:553-581
// as small in-memory mocks. Inside the engine the real headers are used instead.
#pragma once

#include <vector>

#include "lumix_compat.h"

namespace Lumix {

using u64 = uint64_t;

struct PointLight {
	enum Flags : u32 { NONE = 0, CAST_SHADOWS = 1 << 0, DYNAMIC = 1 << 1 };
	Vec3 color;
	float intensity;
	EntityRef entity;
	float fov;
	float attenuation_param;
	float range;
	Flags flags = Flags::NONE;
	u64 guid;
};

struct ReflectionProbe {
	enum Flags { NONE = 0, ENABLED = 1 << 2 };
	u64 guid;
	Flags flags = Flags::NONE;
	u32 size = 128;
	Vec3 half_extents = {100, 100, 100};
	u32 texture_id = 0xffFFffFF;
	void* load_job = nullptr;
};

struct EnvironmentProbe {
	enum Flags { NONE = 0, ENABLED = 1 << 2 };
	Vec3 inner_range;
	Vec3 outer_range;
	Flags flags = Flags::NONE;
	Vec3 sh_coefs[9];
};

struct LightModule { // the light / probe side of RenderModule
	std::vector<PointLight> point_lights; // (the engine's HashMap<EntityRef, PointLight> iterates its values the same way)
	std::vector<EnvironmentProbe> env_probes;
	std::vector<ReflectionProbe> refl_probes;
	std::vector<EntityRef> env_entities, refl_entities;
	const std::vector<PointLight>& getPointLights() { return point_lights; }
	Span<const EnvironmentProbe> getEnvironmentProbes() { return Span<const EnvironmentProbe>(env_probes.data(), env_probes.size()); }
	Span<const ReflectionProbe> getReflectionProbes() { return Span<const ReflectionProbe>(refl_probes.data(), refl_probes.size()); }
	Span<EntityRef> getEnvironmentProbesEntities() { return Span<EntityRef>(env_entities.data(), env_entities.size()); }
	Span<EntityRef> getReflectionProbesEntities() { return Span<EntityRef>(refl_entities.data(), refl_entities.size()); }
};

} // namespace Lumix
