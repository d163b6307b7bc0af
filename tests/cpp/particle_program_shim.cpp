// particle_program_shim.cpp — a C entry point around lumixengine_amd/csrc/lmx_particle_program.cpp for tests/test_particle_program.py
// (the decoder is plain C++ and needs no device; lmx_particles_set_program, which calls it in the product, needs a context).
#include <cstring>

#include "lmx_particle_program.h"

// 0: accepted, 1: refused (LMX_ERR_INVALID), 2: accepted and holds MESH / SPLINE, 3: accepted and holds EMIT (LMX_ERR_UNSUPPORTED both)
extern "C" __attribute__((visibility("default"))) int particle_shim_decode(const uint8_t* bytes, const uint32_t* h, char* err, uint32_t err_cap, uint32_t* n_recs) {
	lmx::ParticleProgramDesc d;
	memset(&d, 0, sizeof(d));
	d.bytes = bytes; d.size = h[0]; d.emit_offset = h[1]; d.output_offset = h[2]; d.channels_count = h[3]; d.registers_count = h[4]; d.outputs_count = h[5];
	d.emit_inputs_count = h[6]; d.n_emitters = h[7]; d.n_globals = h[8];
	lmx::ParticleProgram p;
	std::string e;
	const int rc = lmx::particle_program_decode(d, p, e);
	if (err && err_cap) {
		strncpy(err, e.c_str(), err_cap - 1);
		err[err_cap - 1] = 0;
	}
	if (n_recs) *n_recs = (uint32_t)p.recs.size();
	if (rc != lmx::PD_OK) return 1;
	return p.has_mesh_or_spline ? 2 : p.has_emit ? 3 : 0;
}
