// gpu_pose_processor.h — the PoseProcessor stand-in (C++ host side of include/lumix_mi355.h "pose processor").
//
// In the reference createSortKeys hands every visible skinned model instance to PipelineImpl's PoseProcessor once per frame
// (src/renderer/pipeline.cpp:3889-3898); its jobs allocate a transient GPU slice per batch, fill it with computeSkeletonDualQuats
// (:2680-2745) and leave it in pose->slice (:3730-3787), which createCommands writes into the skinned instance records (:3176-3180).
// GpuPoseProcessor does the same behind lmx_keys_run without the instances ever reaching the host: the list stays on the device,
// lmx_poses_run packs the slices into one buffer of the frame and stores {handle, offset} per entity where lmx_draw_run reads it.
// The absolute poses are the ones PoseBridge::run left in the library.
#pragma once

#include <vector>

#include "lumix_mi355.h"
#include "pose_bridge.h"

namespace Lumix {

struct GpuPoseProcessor {
	explicit GpuPoseProcessor(LmxContext* ctx) : m_ctx(ctx) {}

	// The skin instance of every entity, from the entities PoseBridge::setInstances was given (instance i = its i-th entity);
	// n_entities = the entity range of the sort-key tables (lmx_keys_set_instances). After PoseBridge::setInstances.
	bool setInstances(const PoseBridge& bridge, u32 n_entities) {
		m_skin_of_entity.assign(n_entities, -1);
		const std::vector<EntityRef>& entities = bridge.entities();
		for (u32 i = 0; i < (u32)entities.size(); ++i) {
			const i32 e = entities[i].index;
			if (e >= 0 && (u32)e < n_entities) m_skin_of_entity[e] = (int32_t)i;
		}
		return lmx_poses_set_instances(m_ctx, n_entities, m_skin_of_entity.data()) == LMX_OK;
	}

	// Once per frame, before the first view: handle = gpu::getBindlessHandle(buffer).value of the buffer the renderer binds the frame's
	// dual quaternions through, offset = where the frame's slice starts in it.
	bool beginFrame(u32 handle, u32 offset) { return lmx_poses_begin_frame(m_ctx, handle, offset) == LMX_OK; }

	// After each view's lmx_keys_run (views of a frame append; Pose::frame keeps an instance out of the later views' lists). Enqueues and
	// returns; lmx_keys_sort / lmx_draw_run of the view follow on the same stream.
	bool process() { return lmx_poses_run(m_ctx) == LMX_OK; }

	// {instances, bytes, skipped, overflow} of the frame so far (synchronizes)
	bool counts(LmxPosesCounts& out) { return lmx_poses_counts(m_ctx, &out) == LMX_OK; }

	// the frame's dual quaternions in HBM (to copy or bind behind `handle`) and its counters, stream-ordered behind process()
	bool deviceOutputs(const void** d_dual_quats, const uint32_t** d_counts) { return lmx_poses_device_outputs(m_ctx, d_dual_quats, d_counts) == LMX_OK; }

	const char* lastError() const { return lmx_last_error(m_ctx); }

private:
	LmxContext* m_ctx;
	std::vector<int32_t> m_skin_of_entity;
};

} // namespace Lumix
