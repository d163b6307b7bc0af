"""lumixengine_amd/host/gpu_pose_processor.h - the PoseProcessor stand-in on top of PoseBridge - against the reference's REAL headers
(EntityRef, Model, Pose, RenderModule through pose_bridge.h) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h.
Syntax-only, as tests/test_draw_encoder_compile.py: the engine itself cannot be linked here. The first is skipped where the reference
tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_pose_processor.h"\n'
       "bool use(Lumix::GpuPoseProcessor& p, const Lumix::PoseBridge& b, LmxPosesCounts& c) {\n"
       "\treturn p.setInstances(b, 1000u) && p.beginFrame(7u, 256u) && p.process() && p.counts(c) && p.lastError() != nullptr;\n"
       "}\n")


def test_pose_processor_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "pose_processor_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_pose_processor_compiles_standalone(tmp_path):
    tu = tmp_path / "pose_processor_tu.cpp"
    tu.write_text(USE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
