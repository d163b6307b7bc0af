// lumix_compat_grass.h — what lumixengine_amd/host/gpu_grass.h reads of a Terrain, its textures and grass types, for builds without the
// engine's headers (renderer/terrain.h and renderer/texture.h have the real ones).
#pragma once

#include <vector>

#include "lumix_compat.h"

namespace Lumix {

namespace gpu {
enum class TextureFormat : u32 { R8, RGBA8, R16, SRGBA };
}

enum class GrassRotationMode : i32 { Y_UP, ALL_RANDOM, COUNT };

struct GrassTexture {
	gpu::TextureFormat format = gpu::TextureFormat::RGBA8;
	u32 width = 0, height = 0;
	std::vector<u8> data;
	const u8* getData() const { return data.data(); }
	bool isReady() const { return true; }
};

struct GrassModel {
	bool ready = true;
	bool isReady() const { return ready; }
};

struct Terrain {
	struct GrassType {
		GrassModel* m_grass_model = nullptr;
		float m_spacing = 1, m_distance = 50;
		GrassRotationMode m_rotation_mode = GrassRotationMode::Y_UP;
	};
	i32 m_width = 0, m_height = 0;
	Vec3 m_scale = {1, 1, 1};
	EntityRef m_entity;
	GrassTexture* m_heightmap = nullptr;
	GrassTexture* m_splatmap = nullptr;
	std::vector<GrassType> m_grass_types;
};

struct GrassWorld { // World::getPosition: by entity index, the origin for an entity the test gave no position
	std::vector<DVec3> positions;
	DVec3 getPosition(EntityRef e) const { return e.index >= 0 && (size_t)e.index < positions.size() ? positions[e.index] : DVec3{0, 0, 0}; }
};

} // namespace Lumix
