// lumix_compat_particles.h — what lumixengine_amd/host/gpu_particle_system.h reads of a ParticleSystem and its resource, for builds
// without the engine's headers (renderer/particle_system.h has the real ones).
#pragma once

#include <vector>

#include "lumix_compat.h"

namespace Lumix {

struct ParticleSystemResource {
	struct Emitter {
		std::vector<u8> instructions;
		u32 emit_offset = 0, output_offset = 0, channels_count = 0, update_registers_count = 0, emit_registers_count = 0, output_registers_count = 0, outputs_count = 0,
			init_emit_count = 0, emit_inputs_count = 0, max_ribbons = 0;
		float emit_per_second = 0;
	};
	std::vector<Emitter> m_emitters;
	std::vector<Emitter>& getEmitters() { return m_emitters; }
	bool isReady() const { return true; }
};

struct ParticleWorld {
	DVec3 getPosition(EntityRef) const { return DVec3{0, 0, 0}; }
};

struct ParticleGlobals {
	std::vector<float> v;
	u32 size() const { return (u32)v.size(); }
	const float* begin() const { return v.data(); }
};

struct ParticleSystem {
	ParticleSystemResource* getResource() const { return m_resource; }
	ParticleWorld& m_world;
	EntityPtr m_entity;
	ParticleGlobals m_globals;
	ParticleSystemResource* m_resource = nullptr;
};

} // namespace Lumix
