"""lumixengine_amd/host/gpu_voxels.h - the Voxels stand-in - against the reference's REAL headers (Model, Mesh, AABB, Vec3) under
-DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h + lumix_compat_voxels.h. Syntax-only, as tests/test_grass_compile.py: the
engine itself cannot be linked here. The first is skipped where the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_voxels.h"\n'
       "template <typename ModelT, typename MeshT, typename AABBT> bool use(Lumix::GpuVoxels& v, Lumix::GpuVoxels& w, const ModelT& model, const MeshT& mesh, const AABBT& aabb, Lumix::u8* vb) {\n"
       "\tconst Lumix::Vec3 tri[3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}};\n"
       "\tLumix::u8 voxel; float ao; LmxVoxelsDevice d; LmxVoxelsInfo info; std::vector<Lumix::u8> bytes; std::vector<float> aos;\n"
       "\tv.seed(1u, 2u);\n"
       "\tbool ok = v.voxelize(model, 64u) && v.beginRaster(aabb, 64u) && v.raster(tri, 1u) && v.raster(tri[0], tri[1], tri[2]) && v.raster(mesh);\n"
       "\tok = ok && v.computeAO(32u) && v.blurAO() && v.sample(tri[0], &voxel) && v.sampleAO(tri[1], &ao) && w.set(v);\n"
       "\tok = ok && v.bakeVertexAO(vb, 24u, 10u, 0.3f, vb + 12, 24u) && v.getVoxels(d) && v.getInfo(info) && v.readVoxels(bytes) && v.readAO(aos);\n"
       "\treturn ok && v.lastError() != nullptr && v.handle() != nullptr && d.d_voxels != nullptr;\n"
       "}\n")


def test_voxels_adapter_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "voxels_tu.cpp"
    tu.write_text(USE + "template bool use<Lumix::Model, Lumix::Mesh, Lumix::AABB>(Lumix::GpuVoxels&, Lumix::GpuVoxels&, const Lumix::Model&, const Lumix::Mesh&, const Lumix::AABB&, Lumix::u8*);\n")
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_voxels_adapter_compiles_standalone(tmp_path):
    tu = tmp_path / "voxels_tu.cpp"
    tu.write_text(USE + "template bool use<Lumix::VoxelModel, Lumix::VoxelMesh, Lumix::VoxelAABB>(Lumix::GpuVoxels&, Lumix::GpuVoxels&, const Lumix::VoxelModel&, const Lumix::VoxelMesh&, "
                  "const Lumix::VoxelAABB&, Lumix::u8*);\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
