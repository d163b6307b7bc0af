"""lumixengine_amd/host/gpu_ray_caster.h - the castRay stand-in - against the reference's REAL headers (Ray, RayCastModelHit, Model,
RenderModule) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h + lumix_compat_rays.h. Syntax-only, as
tests/test_cluster_filler_compile.py: the engine itself cannot be linked here. The first is skipped where the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_ray_caster.h"\n'
       "bool use(Lumix::GpuRayCaster& c, Lumix::RenderModule& m, const Lumix::Ray& ray, Lumix::EntityPtr ignored, Lumix::Span<const Lumix::Ray> rays,\n"
       "\tLumix::Span<Lumix::RayCastModelHit> hits, const Lumix::RayCastModelHit& terrain_hit, LmxRaysCounts& n) {\n"
       "\tLumix::RayCastModelHit one = c.castRay(m, ray, ignored, &terrain_hit);\n"
       "\tLumix::GpuRayCaster::merge(one, terrain_hit);\n"
       "\treturn c.reserve(65536u, 1u << 20) && c.castRays(m, rays, hits, ignored) && c.counts(n) && one.is_hit && c.lastError() != nullptr;\n"
       "}\n"
       "Lumix::GpuRayCaster make(LmxContext* ctx, Lumix::ComponentType type) { return Lumix::GpuRayCaster(ctx, type); }\n")


def test_ray_caster_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "ray_caster_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_ray_caster_compiles_standalone(tmp_path):
    tu = tmp_path / "ray_caster_tu.cpp"
    tu.write_text(USE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
