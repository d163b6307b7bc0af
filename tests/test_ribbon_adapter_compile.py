"""lumixengine_amd/host/gpu_particle_system.h with its ribbon calls - emitRibbons, killRibbon, applyTransforms and mirrorRibbons, which
writes Emitter::ribbons and particles_count - against the reference's REAL headers under -DLMX_WITH_LUMIX_HEADERS. Syntax-only, as
tests/test_particle_system_compile.py; skipped where the reference tree is absent. (ParticleSystem keeps m_emitters private: the caller
hands mirrorRibbons the array, as an engine build that befriends it would.)"""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_particle_system.h"\n'
       "bool use(Lumix::GpuParticleSystems& g, Lumix::ParticleSystem& system, Lumix::Array<Lumix::ParticleSystem::Emitter>& emitters, LmxParticlesDevice& d) {\n"
       "\tLumix::u32 index = 0;\n"
       "\tbool ok = g.add(system, 65536u, &index) && g.sync(index, system) && g.applyTransforms() && g.update(1.f / 60);\n"
       "\tok = ok && g.emitRibbons(index, 0, 2) && g.killRibbon(index, 0, 1) && g.mirrorRibbons(index, emitters) && g.fillInstanceData(d);\n"
       "\tfor (const Lumix::ParticleSystem::Emitter& e : system.getEmitters())\n"
       "\t\tfor (const Lumix::ParticleSystem::Ribbon& r : e.ribbons) ok = ok && r.length <= e.particles_count;\n"
       "\treturn ok;\n"
       "}\n")


def test_ribbon_adapter_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "ribbon_adapter_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
