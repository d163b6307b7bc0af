"""lumixengine_amd/host/gpu_ray_caster.h with the procedural-geometry and terrain tables (setProceduralGeometries, setTerrains, setSceneTypes)
against the reference's REAL headers under -DLMX_WITH_LUMIX_HEADERS - ProceduralGeometry, Terrain, Texture and the two maps of RenderModule -
and against tests/cpp/lumix_compat.h + lumix_compat_rays.h + lumix_compat_scene_rays.h. Syntax-only, as tests/test_ray_caster_im_compile.py,
whose translation unit (the calls from before the extension) is compiled along: the extension is additive. The first test is skipped where
the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture
from tests.test_ray_caster_im_compile import USE as USE_BEFORE

USE = (USE_BEFORE +
       "#ifdef LMX_WITH_LUMIX_HEADERS\n"
       "using SceneModule = Lumix::RenderModule;\n"
       "#else\n"
       "using SceneModule = Lumix::SceneRenderModule;\n"
       "#endif\n"
       "bool use_scene(Lumix::GpuRayCaster& c, SceneModule& m, Lumix::ComponentType procedural_geom, Lumix::ComponentType terrain, Lumix::Span<const Lumix::Ray> rays,\n"
       "\tLumix::Span<Lumix::RayCastModelHit> hits, Lumix::EntityPtr ignored, LmxRaysSceneCounts& n) {\n"
       "\tc.setSceneTypes(procedural_geom, terrain);\n"
       "\tif (!c.setProceduralGeometries(m) || !c.setTerrains(m)) return false;\n"
       "\treturn c.castRays(m, rays, hits, ignored) && c.sceneCounts(n) && hits[0].mesh == nullptr && n.overflow == 0u;\n"
       "}\n")


def test_ray_caster_with_scene_tables_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "ray_caster_scene_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_ray_caster_with_scene_tables_compiles_standalone(tmp_path):
    tu = tmp_path / "ray_caster_scene_tu.cpp"
    tu.write_text(USE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
