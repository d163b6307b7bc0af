// gpu_draw_encoder.h — C++ host side of the draw-command path: what PipelineImpl::createCommands (pipeline.cpp:2747-3320) does per run, driven
// by the LmxDrawRun records lmx_draw_run left on the device (include/lumix_mi355.h, "Draw commands").
//
//   createCommands(view) behind the radix sort (pipeline.cpp:1051-1056) + "fill instance data" (:3970-4014)  -> run() + encode()
//
// run() is the device pass; encode() walks the run records and issues per run what the reference's switch issues: useProgram /
// bindIndexBuffer / bindVertexBuffer / drawIndexedInstanced, two draws for a decal run (front part, then the records that intersect the near
// plane with the culling flipped), a gpu::Drawcall for an AUTOINSTANCED run. The instance buffer and the group buffer are bound as two
// buffers the engine owns (the device's outputs copied or imported into them: the graphics-API side of that is the engine's). Strides and
// the back part's offset are those of the records written, not the 36 / 48 / 64 the reference binds.
// Error convention of the reference: no exceptions; a failed call is logged through lastError() and the view draws nothing.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/geometry.h"
	#include "core/math.h"
	#include "renderer/draw_stream.h"
	#include "renderer/gpu/gpu.h"
	#include "renderer/material.h"
	#include "renderer/model.h"
	#include "renderer/render_module.h"
	#include "renderer/shader.h"
#endif

namespace Lumix {

#ifdef LMX_WITH_LUMIX_HEADERS
static_assert(sizeof(ShiftedFrustum) == sizeof(LmxShiftedFrustum), "ShiftedFrustum is 256 bytes");
static_assert(sizeof(Transform) == sizeof(LmxTransform), "Transform is 56 bytes");
#endif
static_assert(sizeof(LmxDrawRun) == 48, "one run record is 48 bytes");

struct GpuDrawEncoder {
	explicit GpuDrawEncoder(LmxContext* ctx) : m_ctx(ctx) {}

	// the device pass for one view, behind lmx_keys_sort; then the run records on the host
	bool run(const double camera_pos[3], const LmxShiftedFrustum& frustum, const uint8_t bucket_depth_sorted[256], uint32_t n_batches) {
		LmxDrawView v;
		memset(&v, 0, sizeof(v));
		memcpy(v.camera_pos, camera_pos, sizeof(v.camera_pos));
		v.frustum = frustum;
		memcpy(v.bucket_depth_sorted, bucket_depth_sorted, 256);
		m_runs.clear();
		if (lmx_draw_run(m_ctx, &v, n_batches) != LMX_OK) return fail("lmx_draw_run");
		if (lmx_draw_counts(m_ctx, &m_counts) != LMX_OK) return fail("lmx_draw_counts");
		m_runs.resize(m_counts.runs);
		if (m_counts.runs && lmx_draw_read_runs(m_ctx, m_runs.data(), m_counts.runs) != LMX_OK) return fail("lmx_draw_read_runs");
		return true;
	}

	const std::vector<LmxDrawRun>& runs() const { return m_runs; }
	const LmxDrawCounts& counts() const { return m_counts; }
	const std::string& lastError() const { return m_error; }

	// device pointers of the last run (instance buffer, group buffer) for the engine's import / copy into its transient buffers
	bool deviceOutputs(const void** d_instance_data, const void** d_group_data) {
		return lmx_draw_device_outputs(m_ctx, nullptr, d_instance_data, d_group_data, nullptr) == LMX_OK || fail("lmx_draw_device_outputs");
	}

#ifdef LMX_WITH_LUMIX_HEADERS
	// What createCommands reads of the pipeline and of a view's bucket (pipeline.cpp:2815-2827, :2763-2786, m_cube_*, m_*_decl)
	struct Bucket {
		DrawStream** substreams; // view.buckets[b].substreams
		u32 define_mask;
		gpu::StateFlags state;
	};
	struct Shared {
		u32 autoinstanced_define_idx, dynamic_define_idx, skinned_define_idx;
		const gpu::VertexDecl* instanced_decl;          // 48 B records
		const gpu::VertexDecl* dyn_instance_decl;       // 96 B
		const gpu::VertexDecl* skinned_instanced_decl;  // 92 B
		const gpu::VertexDecl* decal_decl;
		const gpu::VertexDecl* curve_decal_decl;
		gpu::BufferHandle cube_ib, cube_vb;
		gpu::BufferHandle instance_buffer; u32 instance_buffer_offset; // the view's transient slice holding the instance buffer
		gpu::BufferHandle group_buffer; u32 group_buffer_offset;       // ... and the instancer's group records
	};

	// The walk over the run records: one iteration per draw call of the reference's switch (pipeline.cpp:2829-3317).
	void encode(RenderModule& module, const Bucket* buckets, const Shared& s) {
		Span<ModelInstance> model_instances = module.getModelInstances();
		for (const LmxDrawRun& r : m_runs) {
			const Bucket& b = buckets[r.bucket];
			DrawStream* stream = b.substreams[r.batch];
			const gpu::StateFlags render_state = b.state;
			const u32 vb1_offset = s.instance_buffer_offset + r.data_offset;
			switch (r.kind) {
				case LMX_RUN_AUTOINSTANCED: { // :3005-3035
					if (!r.total_count) break;
					const ModelInstance& mi = model_instances[r.head_entity & 0xffFFff];
					const Mesh& mesh = mi.model->getMesh(r.mesh_idx);
					const Material* material = mi.mesh_materials[r.mesh_idx].material;
					const gpu::StateFlags state = material->m_render_states | render_state;
					const u32 defines = b.define_mask | (1 << s.autoinstanced_define_idx) | material->getDefineMask();
					gpu::Drawcall& dc = stream->draw();
					dc.program = material->getShader()->getProgram(state, mesh.vertex_decl, *s.instanced_decl, defines, mesh.semantics_defines);
					dc.index_buffer = mesh.index_buffer_handle;
					dc.vertex_buffers[0] = mesh.vertex_buffer_handle;
					dc.vertex_buffers[1] = s.group_buffer;
					dc.vertex_buffer_offsets[0] = 0;
					dc.vertex_buffer_offsets[1] = s.group_buffer_offset + r.data_offset;
					dc.vertex_buffer_sizes[0] = mesh.vb_stride;
					dc.vertex_buffer_sizes[1] = r.stride;
					dc.indices_count = mesh.indices_count;
					dc.instances_count = r.total_count;
					dc.index_type = mesh.index_type;
					break;
				}
				case LMX_RUN_MESH:       // :3092-3128
				case LMX_RUN_MOVED_MESH: // :3046-3091
				case LMX_RUN_SKINNED: {  // :3131-3192
					const ModelInstance& mi = model_instances[r.head_entity];
					const Mesh& mesh = mi.meshes[r.mesh_idx];
					const Material* material = mi.mesh_materials[r.mesh_idx].material;
					const gpu::StateFlags state = material->m_render_states | render_state;
					const u32 idx = r.kind == LMX_RUN_MESH ? s.autoinstanced_define_idx : r.kind == LMX_RUN_MOVED_MESH ? s.dynamic_define_idx : s.skinned_define_idx;
					const gpu::VertexDecl& decl = r.kind == LMX_RUN_MESH ? *s.instanced_decl : r.kind == LMX_RUN_MOVED_MESH ? *s.dyn_instance_decl : *s.skinned_instanced_decl;
					const u32 defines = b.define_mask | (1 << idx) | material->getDefineMask();
					stream->useProgram(material->getShader()->getProgram(state, mesh.vertex_decl, decl, defines, mesh.semantics_defines));
					stream->bindIndexBuffer(mesh.index_buffer_handle);
					stream->bindVertexBuffer(0, mesh.vertex_buffer_handle, 0, mesh.vb_stride);
					stream->bindVertexBuffer(1, s.instance_buffer, vb1_offset, r.stride);
					stream->drawIndexedInstanced(mesh.indices_count, r.pair_count, mesh.index_type);
					break;
				}
				case LMX_RUN_DECAL:         // :3193-3253
				case LMX_RUN_CURVE_DECAL: { // :3254-3316
					const EntityRef entity{(i32)r.head_entity};
					const Material* material = r.kind == LMX_RUN_DECAL ? module.getDecal(entity).material : module.getCurveDecal(entity).material;
					const gpu::VertexDecl& decl = r.kind == LMX_RUN_DECAL ? *s.decal_decl : *s.curve_decal_decl;
					stream->bindIndexBuffer(s.cube_ib);
					stream->bindVertexBuffer(0, s.cube_vb, 0, 12);
					gpu::StateFlags state = material->m_render_states | render_state;
					state = state & ~gpu::StateFlags::CULL_FRONT | gpu::StateFlags::CULL_BACK;
					const u32 defines = b.define_mask | material->getDefineMask();
					if (r.front_count) {
						stream->useProgram(material->getShader()->getProgram(state, decl, defines, ""));
						stream->bindVertexBuffer(1, s.instance_buffer, vb1_offset, r.stride);
						stream->drawIndexedInstanced(36, r.front_count, gpu::DataType::U16);
					}
					if (r.pair_count - r.front_count) {
						state = state & ~gpu::StateFlags::DEPTH_FUNCTION;
						state = state & ~gpu::StateFlags::CULL_BACK;
						state = state | gpu::StateFlags::CULL_FRONT;
						stream->useProgram(material->getShader()->getProgram(state, decl, defines, ""));
						stream->bindVertexBuffer(1, s.instance_buffer, vb1_offset + r.stride * r.front_count, r.stride);
						stream->drawIndexedInstanced(36, r.pair_count - r.front_count, gpu::DataType::U16);
					}
					break;
				}
				default: break; // particle / ribbon types: lmx_keys_run never emits them
			}
		}
	}
#endif

private:
	bool fail(const char* what) {
		const char* e = lmx_last_error(m_ctx);
		m_error = std::string(what) + ": " + (e ? e : "");
		return false;
	}

	LmxContext* m_ctx;
	std::vector<LmxDrawRun> m_runs;
	LmxDrawCounts m_counts = {};
	std::string m_error;
};

} // namespace Lumix
