// lumix_compat_scene_rays.h — what gpu_ray_caster.h reads of the engine for procedural geometry and terrains besides lumix_compat.h and
// lumix_compat_rays.h: ProceduralGeometry (renderer/render_module.h:46-64), the gpu enums it names, Texture (renderer/texture.h), Terrain's
// getters (renderer/terrain.h:74-86) and the two maps of RenderModule (:492, :538). Interface mock of the tests, no engine code.
#pragma once

#include <utility>
#include <vector>

#include "lumix_compat.h"

namespace Lumix {

namespace gpu {
enum class PrimitiveType : u32 { TRIANGLES, TRIANGLE_STRIP, LINES, POINTS, NONE };
enum class DataType : u32 { U16, U32 };
enum class TextureFormat : u32 { R8, RGBA8, R16, RGBA16F };
struct VertexDecl {
	PrimitiveType primitive_type = PrimitiveType::TRIANGLES;
	u32 stride = 0;
	u32 getStride() const { return stride; }
};
} // namespace gpu

struct AABB { Vec3 min, max; };
struct ByteStream { // the members of OutputMemoryStream the adapter calls
	std::vector<u8> v;
	const u8* data() const { return v.data(); }
	size_t size() const { return v.size(); }
};
struct ProceduralGeometry {
	ByteStream vertex_data;
	ByteStream index_data;
	gpu::VertexDecl vertex_decl;
	gpu::DataType index_type = gpu::DataType::U16;
	AABB aabb;
	u32 getIndexCount() const { return (u32)(index_data.size() / (index_type == gpu::DataType::U16 ? 2 : 4)); }
};
struct Texture {
	gpu::TextureFormat format = gpu::TextureFormat::R16;
	std::vector<u8> bytes;
	bool ready = true;
	const u8* getData() const { return bytes.data(); }
	bool isReady() const { return ready; }
};
struct Terrain {
	Texture* m_heightmap = nullptr;
	EntityRef m_entity = {};
	Vec3 m_scale = {1, 1, 1};
	i32 m_width = 0, m_height = 0;
	Texture* getHeightmap() const { return m_heightmap; }
	EntityRef getEntity() const { return m_entity; }
	Vec3 getScale() const { return m_scale; }
	int getWidth() const { return m_width; }
	int getHeight() const { return m_height; }
};
// HashMap<K, V> as the adapter walks it: begin() / end() iterators with key() / value(), and `for (V v : map)`
template <typename K, typename V> struct CompatMap {
	std::vector<std::pair<K, V>> items;
	struct Iterator {
		typename std::vector<std::pair<K, V>>::const_iterator it;
		const K& key() { return it->first; }
		const V& value() const { return it->second; }
		const V& operator*() { return it->second; }
		void operator++() { ++it; }
		bool operator!=(const Iterator& o) const { return it != o.it; }
	};
	Iterator begin() const { return Iterator{items.begin()}; }
	Iterator end() const { return Iterator{items.end()}; }
};
struct SceneRenderModule : RenderModule { // renderer/render_module.h:492, :538
	CompatMap<EntityRef, Terrain*> terrains;
	CompatMap<EntityRef, ProceduralGeometry> procedural_geometries;
	const CompatMap<EntityRef, Terrain*>& getTerrains() { return terrains; }
	const CompatMap<EntityRef, ProceduralGeometry>& getProceduralGeometries() { return procedural_geometries; }
};

} // namespace Lumix
