"""lumixengine_amd/host/gpu_particle_system.h with the sources of MESH and SPLINE - add() given the entity's Model, skin instance and Spline,
and the per-frame updateSources() - against the reference's REAL headers (Model, Mesh, Spline) under -DLMX_WITH_LUMIX_HEADERS. Syntax-only,
as tests/test_particle_system_compile.py; skipped where the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_particle_system.h"\n'
       '#include "engine/core.h"\n'
       '#include "renderer/model.h"\n'
       "bool use(Lumix::GpuParticleSystems& g, Lumix::ParticleSystem& system, const Lumix::Model* model, const Lumix::Spline* spline, Lumix::u32 skin_instance) {\n"
       "\tLumix::u32 index = 0;\n"
       "\tbool ok = g.add(system, 65536u, &index, model, skin_instance, spline) && g.sync(index, system) && g.update(1.f / 60);\n"
       "\tok = ok && g.updateSources(index, model, skin_instance, (const Lumix::Spline*)nullptr) && g.updateSources(index, (const Lumix::Model*)nullptr, 0xffffffffu, spline);\n"
       "\treturn ok && g.add(system, 16u) && g.update(1.f / 60);\n"
       "}\n")


def test_source_adapter_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "particle_source_adapter_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
