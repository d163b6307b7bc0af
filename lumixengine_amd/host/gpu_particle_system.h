// gpu_particle_system.h — the ParticleSystem::update / Emitter::fillInstanceData stand-in (C++ host side of include/lumix_mi355.h
// "particle systems").
//
// In the reference RenderModuleImpl::updateParticleSystems calls ParticleSystem::update(dt, page_allocator) for every system and
// Pipeline::setupParticles (src/renderer/pipeline.cpp:2212-2308) asks every emitter for getParticlesDataSizeBytes() and
// fillInstanceData(slice.ptr, ...). GpuParticleSystems keeps the same names over lmx_particles_*: add() registers a ParticleSystem with the
// programs of its resource, update(dt) advances all of them, fillInstanceData() fills every emitter's slice into one device buffer and
// getEmitters(system) names the slices - offset, bytes, particle count on the device, nothing of it read back. Ribbon emitters are taken
// with their options; emitRibbons, killRibbon and applyTransforms forward ParticleSystem's calls of those names, and mirrorRibbons copies
// the ribbon records (host state of the library: no wait) into Emitter::ribbons and particles_count, so that the ribbon loops of
// Pipeline's createCommands (pipeline.cpp:2865, :2919) draw from the device slice unchanged - the slice is packed per ribbon, which is
// the layout those loops assume. MESH / SPLINE programs are taken when add() is given what they read of the system's entity - its Model
// (mesh 0 and its skin, uploaded once per model), the skin instance the pose bridge gave the entity and its Spline; updateSources()
// re-declares them for an entity whose pose instance or spline changed. Autodestroy and the sort-key pairs stay with the engine: add()
// returns false for a system it cannot take and the engine keeps updating that one itself (a system refused at its programs keeps its
// index, with empty programs).
//
// `System` is ParticleSystem inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any type with getResource(),
// m_globals, m_world and m_entity (tests/cpp/lumix_compat_particles.h).
#pragma once

#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/math.h"
	#include "engine/world.h"
	#include "renderer/particle_system.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_particles.h"
#endif

namespace Lumix {

struct GpuParticleSystems {
	// What Pipeline::setupParticles needs of an emitter: where its slice lies in the frame buffer. `slice` is a DEVICE pointer into d_slices.
	struct Emitter {
		u32 global_index;              // into LmxParticlesDevice::d_slices / d_counts
		u32 outputs_count;
		const LmxParticleSlice* slice; // {offset, bytes = getParticlesDataSizeBytes(), particles} of the last fillInstanceData()
	};

	explicit GpuParticleSystems(LmxContext* ctx) : m_ctx(ctx) { lmx_particles_create(ctx, &m_ps); }
	~GpuParticleSystems() { lmx_particles_destroy(m_ps); }
	GpuParticleSystems(const GpuParticleSystems&) = delete;
	void operator=(const GpuParticleSystems&) = delete;

	// Registers `system` (its resource must be ready) with `capacity` particles per emitter. False: the system stays with the engine.
	template <typename System> bool add(System& system, u32 capacity, u32* out_index = nullptr) {
		return addDeclared(system, capacity, out_index, [](u32) { return true; });
	}

	// ... with what MESH and SPLINE read of the system's entity, from the engine's objects: `model` = RenderModule::getModelInstanceModel(entity)
	// (null: no model instance), `skin_instance` = the instance of lmx_skin_set_instances the pose bridge gave the entity (0xffffffff: no
	// pose), `spline` = &CoreModule::getSpline(entity) where the entity has the component (null: none). A system whose programs hold MESH or
	// SPLINE is taken only through this overload. False also for a spline of one or two points (the reference reads outside its array).
	template <typename System, typename Model, typename Spline> bool add(System& system, u32 capacity, u32* out_index, const Model* model, u32 skin_instance, const Spline* spline) {
		return addDeclared(system, capacity, out_index, [&](u32 index) { return updateSources(index, model, skin_instance, spline); });
	}

	// Per frame, for a system whose entity got another pose instance, model or spline: the tables follow in stream order, no new layout and
	// no reset (a new POSE of the same instance needs no call: the palette is read where lmx_skin_run leaves it).
	template <typename Model, typename Spline> bool updateSources(u32 index, const Model* model, u32 skin_instance, const Spline* spline) {
		LmxParticleMeshSource src = {0xffffffffu, skin_instance, 0};
		if (model && model->isReady() && model->getMeshCount() > 0) {
			const auto& mesh = model->getMesh(0);
			const bool bones = model->getBones().size() > 0;
			static_assert(sizeof(mesh.vertices[0]) == 3 * sizeof(float) && sizeof(mesh.skin[0]) == sizeof(LmxSkin), "Mesh::vertices / Mesh::skin are read as they lie");
			if (bones && mesh.skin.size() != mesh.vertices.size()) return false;
			u32 id = 0xffffffffu;
			for (const ModelMesh& m : m_meshes)
				if (m.model == (const void*)model) id = m.mesh;
			if (id == 0xffffffffu) { // once per model, whatever number of systems sit on it
				if (mesh.vertices.size() == 0) return false;
				const LmxSkin* skin = mesh.skin.size() == mesh.vertices.size() ? (const LmxSkin*)&mesh.skin[0] : nullptr;
				if (lmx_particles_add_mesh(m_ps, (u32)mesh.vertices.size(), (const float*)&mesh.vertices[0], skin, &id) != LMX_OK) return false;
				m_meshes.push_back(ModelMesh{(const void*)model, id});
			}
			src.mesh = id;
			src.flags = bones ? (u32)LMX_PARTICLE_MESH_HAS_BONES : 0u;
		}
		if (lmx_particles_set_mesh_source(m_ps, index, &src) != LMX_OK) return false;
		const u32 n_points = spline ? (u32)spline->points.size() : 0u;
		if (n_points == 1 || n_points == 2) return false;
		return lmx_particles_set_spline(m_ps, index, n_points ? (const float*)&spline->points[0] : nullptr, n_points) == LMX_OK;
	}

private:
	struct ModelMesh { const void* model; u32 mesh; };
	std::vector<ModelMesh> m_meshes;

	// `declare(index)` runs behind lmx_particles_add_system and before the programs are set: a declaration is what lets a program hold MESH / SPLINE
	template <typename System, typename Declare> bool addDeclared(System& system, u32 capacity, u32* out_index, Declare declare) {
		auto* res = system.getResource();
		if (!res || !res->isReady()) return false;
		auto& emitters = res->getEmitters();
		for (const auto& e : emitters)
			if (e.max_ribbons > 0 && !hasRibbonFields(e, 0)) return false; // a resource type without the ribbon fields: stays with the engine
		u32 index = 0;
		if (lmx_particles_add_system(m_ps, (u32)emitters.size(), (u32)system.m_globals.size(), &index) != LMX_OK) return false;
		m_first.push_back((u32)m_emitters.size());
		bool ok = declare(index);
		u32 k = 0;
		for (const auto& e : emitters) {
			LmxParticleProgram p;
			p.instructions = (const uint8_t*)e.instructions.data();
			p.size = (u32)e.instructions.size();
			p.emit_offset = e.emit_offset; p.output_offset = e.output_offset;
			p.channels_count = e.channels_count;
			p.registers_count = e.update_registers_count > e.output_registers_count ? e.update_registers_count : e.output_registers_count;
			if (e.emit_registers_count > p.registers_count) p.registers_count = e.emit_registers_count;
			p.outputs_count = e.outputs_count; p.emit_inputs_count = e.emit_inputs_count;
			p.init_emit_count = e.init_emit_count; p.emit_per_second = e.emit_per_second;
			LmxParticleEmitterOptions o = {};
			o.max_ribbons = e.max_ribbons;
			ribbonOptions(e, o, 0);
			ok = ok && lmx_particles_set_program(m_ps, index, k, &p) == LMX_OK && lmx_particles_set_emitter_options(m_ps, index, k, &o) == LMX_OK;
			if (e.max_ribbons == 0) ok = ok && lmx_particles_reserve(m_ps, index, k, capacity) == LMX_OK; // (a ribbon emitter's capacity is max_ribbons x max_ribbon_length)
			checkStride(e, 0);
			m_emitters.push_back(Emitter{(u32)m_emitters.size(), e.outputs_count, nullptr});
			++k;
		}
		m_positions.resize(3 * (size_t)(index + 1));
		if (out_index) *out_index = index;
		if (!ok) { // a program was refused (MESH, SPLINE, malformed): the system stays registered but inert - empty programs, no capacity -
			// so the others go on; the engine keeps updating this one itself
			static const uint8_t nothing[3] = {0, 0, 0}; // END | END | END
			LmxParticleProgram p = {};
			p.instructions = nothing; p.size = 3; p.emit_offset = 1; p.output_offset = 2;
			const LmxParticleEmitterOptions none = {};
			for (u32 e = 0; e < k; ++e) {
				lmx_particles_set_emitter_options(m_ps, index, e, &none);
				lmx_particles_set_program(m_ps, index, e, &p);
				lmx_particles_reserve(m_ps, index, e, 0);
			}
		}
		return ok;
	}

public:
	// ParticleSystem::m_globals and World::getPosition(entity) of a registered system, before update()
	template <typename System> bool sync(u32 index, System& system) {
		const DVec3 pos = system.m_world.getPosition(EntityRef{system.m_entity.index});
		m_positions[3 * (size_t)index] = pos.x; m_positions[3 * (size_t)index + 1] = pos.y; m_positions[3 * (size_t)index + 2] = pos.z;
		return lmx_particles_set_globals(m_ps, index, system.m_globals.begin(), (u32)system.m_globals.size()) == LMX_OK;
	}

	// ParticleSystem::update(dt, page_allocator) of every registered system: enqueues and returns
	bool update(float dt) {
		if (lmx_particles_set_entity_positions(m_ps, (u32)(m_positions.size() / 3), m_positions.data()) != LMX_OK) return false;
		return lmx_particles_step(m_ps, dt) == LMX_OK;
	}

	// Emitter::fillInstanceData of every emitter into the frame buffer: enqueues and returns; `out` names the buffer
	bool fillInstanceData(LmxParticlesDevice& out) {
		if (lmx_particles_fill(m_ps) != LMX_OK || lmx_particles_device_outputs(m_ps, &out) != LMX_OK) return false;
		for (Emitter& e : m_emitters) e.slice = out.d_slices + e.global_index;
		return true;
	}

	// ParticleSystem::getEmitters() of a registered system
	Span<const Emitter> getEmitters(u32 index) const {
		const u32 first = m_first[index], end = index + 1 < (u32)m_first.size() ? m_first[index + 1] : (u32)m_emitters.size();
		return Span<const Emitter>(m_emitters.data() + first, (uint64_t)(end - first));
	}

	// ParticleSystem::emitRibbons / killRibbon of a registered system: enqueued in stream order
	bool emitRibbons(u32 index, u32 emitter, u32 num_ribbons) { return lmx_particles_emit_ribbons(m_ps, index, emitter, num_ribbons) == LMX_OK; }
	bool killRibbon(u32 index, u32 emitter, u32 ribbon) { return lmx_particles_kill_ribbon(m_ps, index, emitter, ribbon) == LMX_OK; }

	// ParticleSystem::applyTransform of every registered system with the positions of the last sync(): emission on movement
	bool applyTransforms() { return lmx_particles_apply_transforms(m_ps, (u32)(m_positions.size() / 3), m_positions.data()) == LMX_OK; }

	// Emitter::ribbons and particles_count of every ribbon emitter of a registered system, as the calls so far left them (no wait): the
	// engine's ribbon loops read ribbon.length and advance by length x stride, which is LmxParticleRibbon::points_offset.
	// `emitters` is the system's own Array<Emitter> (ParticleSystem keeps it private: the engine build befriends the caller).
	template <typename Emitters> bool mirrorRibbons(u32 index, Emitters& emitters) {
		bool ok = true;
		u32 k = 0;
		for (auto& e : emitters) {
			if (e.resource_emitter.max_ribbons > 0) {
				u32 n = 0;
				m_ribbons.resize(e.resource_emitter.max_ribbons);
				ok = ok && lmx_particles_ribbons(m_ps, index, k, m_ribbons.data(), (u32)m_ribbons.size(), &n) == LMX_OK;
				e.ribbons.resize(ok ? n : 0);
				u32 total = 0;
				for (u32 r = 0; r < (u32)e.ribbons.size(); ++r) {
					e.ribbons[r].offset = m_ribbons[r].offset; e.ribbons[r].length = m_ribbons[r].length; e.ribbons[r].emit_index = m_ribbons[r].emit_index;
					total += m_ribbons[r].length;
				}
				e.particles_count = total;
			}
			++k;
		}
		return ok;
	}

	bool reset(u32 index) { return lmx_particles_reset(m_ps, index) == LMX_OK; } // ParticleSystem::reset
	const char* lastError() const { return lmx_last_error(m_ctx); }
	LmxParticles* handle() const { return m_ps; }

private:
	// The ribbon fields of ParticleSystemResource::Emitter, where the resource type has them (the engine's does)
	template <typename E> static auto hasRibbonFields(const E& e, int) -> decltype(e.max_ribbon_length, e.init_ribbons_count, e.emit_move_distance, true) { return true; }
	template <typename E> static bool hasRibbonFields(const E&, long) { return false; }
	template <typename E> static auto ribbonOptions(const E& e, LmxParticleEmitterOptions& o, int) -> decltype(e.max_ribbon_length, e.init_ribbons_count, e.tube_segments, e.emit_move_distance, void()) {
		o.max_ribbon_length = e.max_ribbon_length; o.init_ribbons_count = e.init_ribbons_count; o.tube_segments = e.tube_segments;
		o.emit_move_distance = e.emit_move_distance;
	}
	template <typename E> static void ribbonOptions(const E&, LmxParticleEmitterOptions&, long) {}
	// the renderer reads the slice with the emitter's vertex declaration: one float per output
	template <typename E> static auto checkStride(const E& e, int) -> decltype(e.vertex_decl.getStride(), void()) { ASSERT(e.vertex_decl.getStride() == e.outputs_count * sizeof(float)); }
	template <typename E> static void checkStride(const E&, long) {}

	std::vector<LmxParticleRibbon> m_ribbons;
	LmxContext* m_ctx;
	LmxParticles* m_ps = nullptr;
	std::vector<u32> m_first;
	std::vector<Emitter> m_emitters;
	std::vector<double> m_positions;
};

} // namespace Lumix
