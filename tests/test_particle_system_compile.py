"""lumixengine_amd/host/gpu_particle_system.h - the ParticleSystem::update / fillInstanceData stand-in - against the reference's REAL headers
(ParticleSystem, ParticleSystemResource, World) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h +
lumix_compat_particles.h. Syntax-only, as tests/test_cluster_filler_compile.py: the engine itself cannot be linked here. The first is
skipped where the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_particle_system.h"\n'
       "bool use(Lumix::GpuParticleSystems& g, Lumix::ParticleSystem& system, LmxParticlesDevice& d) {\n"
       "\tLumix::u32 index = 0;\n"
       "\tbool ok = g.add(system, 65536u, &index) && g.sync(index, system) && g.update(1.f / 60) && g.fillInstanceData(d);\n"
       "\tfor (const Lumix::GpuParticleSystems::Emitter& e : g.getEmitters(index)) ok = ok && e.slice != nullptr && e.outputs_count > 0;\n"
       "\treturn ok && g.reset(index) && g.lastError() != nullptr && g.handle() != nullptr;\n"
       "}\n")


def test_particle_system_adapter_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "particle_system_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_particle_system_adapter_compiles_standalone(tmp_path):
    tu = tmp_path / "particle_system_tu.cpp"
    tu.write_text(USE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
