// gpu_instanced_models.h — C++ host side of the instanced-model path: RenderModule's InstancedModel hooks on an MI355X through the C ABI
// of liblumix_mi355.so (include/lumix_mi355.h, "Instanced models").
//
//   RenderModuleImpl::endInstancedModelEditing / initInstancedModelGPUData (render_module.cpp:1280-1365) -> endInstancedModelEditing()
//   PipelineImpl::encodeInstancedModels(stream, view) (pipeline.cpp:2449-2660)                          -> encodeInstancedModels()
//
// One slot per instanced model, in the order the engine registers them (the entity is the key). The draw loop of encodeInstancedModels
// stays in the engine: it binds deviceOutputs()' record buffer as the instance stream and issues drawIndirect at (indirect_offset + i).
// Error convention of the reference: no exceptions; a failed call is logged through lastError() and the frame draws nothing for it.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/allocator.h"
	#include "core/geometry.h"
	#include "core/math.h"
	#include "engine/world.h"
	#include "renderer/model.h"
	#include "renderer/render_module.h"
#endif

namespace Lumix {

#ifdef LMX_WITH_LUMIX_HEADERS
// the records go to the device as they are: InstancedModel::InstanceData must be LmxImInstance byte for byte
static_assert(sizeof(InstancedModel::InstanceData) == sizeof(LmxImInstance), "InstancedModel::InstanceData is 32 bytes");
static_assert(offsetof(InstancedModel::InstanceData, lod) == offsetof(LmxImInstance, lod), "InstanceData::lod");
static_assert(offsetof(InstancedModel::InstanceData, pos) == offsetof(LmxImInstance, pos), "InstanceData::pos");
static_assert(offsetof(InstancedModel::InstanceData, scale) == offsetof(LmxImInstance, scale), "InstanceData::scale");
static_assert(sizeof(ShiftedFrustum) == sizeof(LmxShiftedFrustum), "ShiftedFrustum is 256 bytes");
static_assert(sizeof(LODMeshIndices) == sizeof(LmxLodIndices), "LODMeshIndices is {from, to}");
#endif

struct GpuInstancedModels {
	explicit GpuInstancedModels(LmxContext* ctx) : m_ctx(ctx) {
		if (lmx_im_create(ctx, &m_im) != LMX_OK) fail("lmx_im_create");
	}
	~GpuInstancedModels() {
		if (m_im) lmx_im_destroy(m_im);
	}
	GpuInstancedModels(const GpuInstancedModels&) = delete;
	GpuInstancedModels& operator=(const GpuInstancedModels&) = delete;

	// the model's slot, registered on first use (entity = the InstancedModel's key in RenderModuleImpl::m_instanced_models)
	int slotOf(int32_t entity) {
		for (size_t i = 0; i < m_entities.size(); ++i)
			if (m_entities[i] == entity) return (int)i;
		return -1;
	}

	// Model data + instances of one InstancedModel (endInstancedModelEditing -> initInstancedModelGPUData): the grid is built on the device
	bool endInstancedModelEditing(int32_t entity, const float lod_distances[4], const LmxLodIndices lod_indices[5], float origin_radius, uint32_t mesh_count,
		const uint32_t* indices_count, uint32_t n, const LmxImInstance* instances) {
		if (!m_im) return false;
		int slot = slotOf(entity);
		const uint32_t model = slot < 0 ? (uint32_t)m_entities.size() : (uint32_t)slot;
		lmx_ctx_lock(m_ctx);
		int rc = lmx_im_set_model(m_im, model, lod_distances, lod_indices, origin_radius, mesh_count, indices_count);
		if (rc == LMX_OK && slot < 0) {
			m_entities.push_back(entity);
			m_origins.resize(3 * m_entities.size(), 0.0);
		}
		if (rc == LMX_OK) rc = lmx_im_set_instances(m_im, model, n, instances);
		lmx_ctx_unlock(m_ctx);
		return rc == LMX_OK || fail("lmx_im_set_model / lmx_im_set_instances");
	}

	// RenderModule::destroyInstancedModel, or a Model that is not ready (encodeInstancedModels skips `!m || !m->isReady()`): the model keeps its
	// slot (ids are dense) with no instance - it emits nothing and its indirect records draw 0 instances
	bool destroyInstancedModel(int32_t entity) {
		const int slot = slotOf(entity);
		if (!m_im || slot < 0) return false;
		lmx_ctx_lock(m_ctx);
		const int rc = lmx_im_set_instances(m_im, (uint32_t)slot, 0, nullptr);
		lmx_ctx_unlock(m_ctx);
		return rc == LMX_OK || fail("lmx_im_set_instances");
	}

	// World::getTransform(entity).pos of a registered model (before the frame's first encodeInstancedModels)
	void setOrigin(int32_t entity, const double pos[3]) {
		const int slot = slotOf(entity);
		if (slot < 0) return;
		for (int k = 0; k < 3; ++k) m_origins[3 * (size_t)slot + k] = pos[k];
		m_origins_dirty = true;
	}

	// encodeInstancedModels(view) for every registered model: the view's bin records and indirect records stay in HBM (deviceOutputs)
	bool encodeInstancedModels(uint32_t view_slot, const double camera_pos[3], const LmxShiftedFrustum& frustum, float lod_multiplier, float time_delta,
		bool is_shadow) {
		if (!m_im) return false;
		LmxImView v;
		memset(&v, 0, sizeof(v));
		for (int k = 0; k < 3; ++k) v.camera_pos[k] = camera_pos[k];
		v.lod_multiplier = lod_multiplier;
		v.time_delta = time_delta;
		v.is_shadow = is_shadow ? 1u : 0u;
		lmx_ctx_lock(m_ctx);
		int rc = LMX_OK;
		if (m_origins_dirty) rc = lmx_im_set_origins(m_im, (uint32_t)m_entities.size(), m_origins.data());
		m_origins_dirty = rc != LMX_OK;
		if (rc == LMX_OK) rc = lmx_im_run(m_im, view_slot, &v, &frustum);
		lmx_ctx_unlock(m_ctx);
		return rc == LMX_OK || fail("lmx_im_run");
	}

	bool deviceOutputs(uint32_t view_slot, const void** d_records, const void** d_indirect, const void** d_counts) {
		return m_im && lmx_im_device_outputs(m_im, view_slot, d_records, d_indirect, d_counts) == LMX_OK;
	}

#ifdef LMX_WITH_LUMIX_HEADERS
	// The engine's types: InstancedModel + its Model (getLODDistances, getLODIndices, getOriginBoundingRadius, Mesh::indices_count)
	bool endInstancedModelEditing(EntityRef entity, const InstancedModel& im, const Model& model) {
		LmxLodIndices lod[5];
		memcpy(lod, model.getLODIndices(), sizeof(lod));
		uint32_t indices[LMX_IM_MAX_MESHES + 1];
		const uint32_t mesh_count = (uint32_t)model.getMeshCount();
		for (uint32_t i = 0; i < mesh_count && i <= LMX_IM_MAX_MESHES; ++i) indices[i] = (uint32_t)model.getMesh(i).indices_count;
		return endInstancedModelEditing(entity.index, model.getLODDistances(), lod, model.getOriginBoundingRadius(), mesh_count, indices,
			(uint32_t)im.instances.size(), reinterpret_cast<const LmxImInstance*>(im.instances.begin()));
	}
	void setOrigin(EntityRef entity, const World& world) {
		const DVec3 p = world.getTransform(entity).pos;
		const double pos[3] = {p.x, p.y, p.z};
		setOrigin(entity.index, pos);
	}
	// view.cp.pos, view.cp.frustum, view.cp.is_shadow of PipelineImpl's View (CameraParams, renderer/pipeline.h:20-30)
	bool encodeInstancedModels(uint32_t view_slot, const DVec3& camera_pos, const ShiftedFrustum& frustum, bool is_shadow, float lod_multiplier, float time_delta) {
		const double pos[3] = {camera_pos.x, camera_pos.y, camera_pos.z};
		return encodeInstancedModels(view_slot, pos, reinterpret_cast<const LmxShiftedFrustum&>(frustum), lod_multiplier, time_delta, is_shadow);
	}
#endif

	// For the ray casts (gpu_ray_caster.h): the C-ABI object, the registered entities in slot order, and the origins brought up to date
	LmxInstancedModels* handle() const { return m_im; }
	const std::vector<int32_t>& entities() const { return m_entities; }
	bool flushOrigins() {
		if (!m_im || !m_origins_dirty) return m_im != nullptr;
		lmx_ctx_lock(m_ctx);
		const int rc = lmx_im_set_origins(m_im, (uint32_t)m_entities.size(), m_origins.data());
		lmx_ctx_unlock(m_ctx);
		m_origins_dirty = rc != LMX_OK;
		return rc == LMX_OK || fail("lmx_im_set_origins");
	}

	const std::string& lastError() const { return m_error; }

private:
	bool fail(const char* what) {
		m_error = std::string(what) + ": " + lmx_last_error(m_ctx);
		return false;
	}

	LmxContext* m_ctx = nullptr;
	LmxInstancedModels* m_im = nullptr;
	std::vector<int32_t> m_entities;
	std::vector<double> m_origins;
	bool m_origins_dirty = false;
	std::string m_error;
};

} // namespace Lumix
