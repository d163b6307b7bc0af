"""lumixengine_amd/host/gpu_ray_caster.h with the instanced models attached (setInstancedModels over gpu_instanced_models.h) against the
reference's REAL headers under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h + lumix_compat_rays.h. Syntax-only, as
tests/test_ray_caster_compile.py, whose translation unit (the calls from before the extension) is compiled along: the extension is
additive. The first test is skipped where the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture
from tests.test_ray_caster_compile import USE as USE_BEFORE

USE = (USE_BEFORE +
       "bool use_im(Lumix::GpuRayCaster& c, Lumix::GpuInstancedModels& im, Lumix::RenderModule& m, Lumix::ComponentType instanced_model, const Lumix::i32* ray_model,\n"
       "\tLumix::Model* const* models, Lumix::Span<const Lumix::Ray> rays, Lumix::Span<Lumix::RayCastModelHit> hits, Lumix::EntityPtr ignored, LmxRaysImCounts& n) {\n"
       "\tconst double origin[3] = {1.0e6, 50.0, -1.0e6};\n"
       "\tim.setOrigin(3, origin);\n"
       "\tif (!c.setInstancedModels(&im, instanced_model, ray_model, models)) return false;\n"
       "\tconst bool ok = c.castRays(m, rays, hits, ignored) && c.imCounts(n) && hits[0].subindex == 0u && im.handle() != nullptr && im.entities().empty();\n"
       "\treturn c.setInstancedModels(nullptr, instanced_model, nullptr, nullptr) && ok;\n"
       "}\n")


def test_ray_caster_with_instanced_models_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "ray_caster_im_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_ray_caster_with_instanced_models_compiles_standalone(tmp_path):
    tu = tmp_path / "ray_caster_im_tu.cpp"
    tu.write_text(USE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
