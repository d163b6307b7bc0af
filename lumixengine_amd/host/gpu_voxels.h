// gpu_voxels.h — the Voxels stand-in (C++ host side of include/lumix_mi355.h "Voxels"), with the reference's member names.
//
// In the reference Voxels (src/renderer/voxels.h) is used by ModelImporter::bakeVertexAO (renderer/editor/model_importer.cpp:1290-1351:
// beginRaster(aabb, 64), raster of every triangle, computeAO(32), blurAO, sampleAO per vertex) and by the voxelizer tool
// (renderer/editor/voxelizer_ui.cpp: voxelize(model, max_res), computeAO, blurAO, then a draw of the voxels). GpuVoxels keeps those
// members over lmx_voxels_*:
//   beginRaster(aabb, max_res)       a cleared grid
//   raster(triangles, n)             n triangles of three Vec3 each, added to the grid (one launch, not one call per triangle)
//   raster(mesh)                     every triangle of a Mesh
//   voxelize(model, max_res)         the AABB over the referenced vertices, beginRaster, every mesh of the model
//   computeAO(ray_count)             continues the generator this object holds (seed(u, v) sets it; the reference seeds from the clock)
//   blurAO(), sample(p, out), sampleAO(p, out), set(rhs)
//   bakeVertexAO(positions, stride, n, min_ao, out, out_stride)   bakeVertexAO's last loop: one u8 per vertex inside the grid
//   getVoxels(out)                   device pointers and host copies for the tool's draw
// Every member returns false where the library refuses (lastError() says why): the caller then runs the engine's own Voxels.
// The lazy single-point computeAO(const Vec3&, u32) has no counterpart: nothing in the reference calls it.
//
// `ModelT` / `MeshT` / `AABBT` are Model, Mesh and AABB inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any types
// with the members read here (tests/cpp/lumix_compat_voxels.h).
#pragma once

#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/geometry.h"
	#include "core/math.h"
	#include "renderer/model.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_voxels.h"
#endif

namespace Lumix {

static_assert(sizeof(Vec3) == 12, "a triangle is nine floats");

struct GpuVoxels {
	explicit GpuVoxels(LmxContext* ctx) : m_ctx(ctx) { lmx_voxels_create(ctx, &m_voxels); }
	~GpuVoxels() { lmx_voxels_destroy(m_voxels); }
	GpuVoxels(const GpuVoxels&) = delete;
	void operator=(const GpuVoxels&) = delete;

	void seed(u32 u, u32 v) { m_u = u; m_v = v; } // RandomGenerator(u, v): neither half may be 0

	bool set(const GpuVoxels& rhs) {
		m_u = rhs.m_u; m_v = rhs.m_v;
		return lmx_voxels_set(m_voxels, rhs.m_voxels) == LMX_OK;
	}

	template <typename AABBT> bool beginRaster(const AABBT& aabb, u32 max_res) {
		const float mn[3] = {aabb.min.x, aabb.min.y, aabb.min.z}, mx[3] = {aabb.max.x, aabb.max.y, aabb.max.z};
		return lmx_voxels_begin_raster(m_voxels, mn, mx, max_res) == LMX_OK;
	}

	// n triangles, three corners each
	bool raster(const Vec3* triangles, u32 n) {
		m_indices.resize(3 * (size_t)n);
		for (size_t i = 0; i < m_indices.size(); ++i) m_indices[i] = (u32)i;
		return lmx_voxels_raster(m_voxels, triangles, sizeof(Vec3), 3 * n, m_indices.data(), 4, 3 * n) == LMX_OK;
	}
	bool raster(const Vec3& a, const Vec3& b, const Vec3& c) {
		const Vec3 tri[3] = {a, b, c};
		return raster(tri, 1);
	}
	template <typename MeshT> bool raster(const MeshT& mesh) {
		const LmxVoxelsMesh m = describe(mesh);
		return lmx_voxels_raster(m_voxels, m.positions, m.stride_bytes, m.n_vertices, m.indices, m.index_bytes, m.index_count) == LMX_OK;
	}

	template <typename ModelT> bool voxelize(const ModelT& model, u32 max_res) {
		if (!model.isReady()) return false;
		m_meshes.clear();
		for (u32 i = 0; i < (u32)model.getMeshCount(); ++i) m_meshes.push_back(describe(model.getMesh(i)));
		return lmx_voxels_voxelize(m_voxels, m_meshes.data(), (u32)m_meshes.size(), max_res) == LMX_OK;
	}

	bool computeAO(u32 ray_count) {
		if (lmx_voxels_compute_ao(m_voxels, ray_count, m_u, m_v) != LMX_OK) return false;
		return lmx_voxels_rng_state(m_voxels, &m_u, &m_v) == LMX_OK; // the next call continues the stream
	}
	bool blurAO() { return lmx_voxels_blur_ao(m_voxels) == LMX_OK; }

	bool sample(const Vec3& p, u8* out) const {
		u8 inside = 0;
		return lmx_voxels_sample(m_voxels, &p.x, 1, out, &inside) == LMX_OK && inside != 0;
	}
	bool sampleAO(const Vec3& p, float* out) const {
		u8 inside = 0;
		return lmx_voxels_sample_ao(m_voxels, &p.x, 1, out, &inside) == LMX_OK && inside != 0;
	}

	// bakeVertexAO's last loop for one vertex buffer: positions at `positions + i * stride`, the AO byte written to `out + i * out_stride`
	// for every vertex inside the grid
	bool bakeVertexAO(const u8* positions, u32 stride, u32 n, float min_ao, u8* out, u32 out_stride) {
		m_bytes.resize(n);
		for (u32 i = 0; i < n; ++i) m_bytes[i] = out[(size_t)i * out_stride];
		if (lmx_voxels_bake_vertex_ao(m_voxels, positions, stride, n, min_ao, m_bytes.data()) != LMX_OK) return false;
		for (u32 i = 0; i < n; ++i) out[(size_t)i * out_stride] = m_bytes[i];
		return true;
	}

	bool getInfo(LmxVoxelsInfo& out) const { return lmx_voxels_info(m_voxels, &out) == LMX_OK; }
	bool getVoxels(LmxVoxelsDevice& out) const { return lmx_voxels_device_outputs(m_voxels, &out) == LMX_OK; }
	// m_voxels / m_ao on the host, for the tool's cube draw
	bool readVoxels(std::vector<u8>& out) const {
		LmxVoxelsInfo info;
		if (!getInfo(info)) return false;
		out.resize((size_t)info.resolution[0] * info.resolution[1] * info.resolution[2]);
		return lmx_voxels_read(m_voxels, out.data(), (u32)out.size()) == LMX_OK;
	}
	bool readAO(std::vector<float>& out) const {
		LmxVoxelsInfo info;
		if (!getInfo(info)) return false;
		out.resize((size_t)info.resolution[0] * info.resolution[1] * info.resolution[2]);
		return lmx_voxels_read_ao(m_voxels, out.data(), (u32)out.size()) == LMX_OK;
	}

	const char* lastError() const { return lmx_last_error(m_ctx); }
	LmxVoxels* handle() const { return m_voxels; }

private:
	template <typename MeshT> static LmxVoxelsMesh describe(const MeshT& mesh) { // forEachTriangle's view of a Mesh (voxels.cpp:8-31)
		LmxVoxelsMesh m;
		m.positions = mesh.vertices.begin();
		m.stride_bytes = sizeof(Vec3);
		m.n_vertices = (u32)mesh.vertices.size();
		m.indices = mesh.indices.data();
		m.index_bytes = mesh.areIndices16() ? 2 : 4;
		m.index_count = (u32)mesh.indices_count;
		return m;
	}

	LmxContext* m_ctx;
	LmxVoxels* m_voxels = nullptr;
	u32 m_u = 521288629, m_v = 362436069; // RandomGenerator's default arguments (core/math.h:575)
	std::vector<u32> m_indices;
	std::vector<LmxVoxelsMesh> m_meshes;
	std::vector<u8> m_bytes;
};

} // namespace Lumix
