// lumix_compat_rays.h — what gpu_ray_caster.h reads of the engine besides lumix_compat.h: Ray (core/geometry.h:12-15), ComponentType
// (engine/component_types: an index) and RayCastModelHit (renderer/model.h:45-55). Interface mock of the tests, no engine code.
#pragma once

#include "lumix_compat.h"

namespace Lumix {

struct Ray { DVec3 origin; Vec3 dir; };
struct ComponentType { int index = -1; };
struct RayCastModelHit {
	bool is_hit;
	float t;
	DVec3 origin;
	Vec3 dir;
	Mesh* mesh;
	EntityPtr entity;
	ComponentType component_type;
	u32 subindex;
};

} // namespace Lumix
