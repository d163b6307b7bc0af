"""lumixengine_amd/host/gpu_animator.h - the evalBlendStack stand-in of AnimationModuleImpl::updateAnimator - against the reference's REAL
headers (anim::RuntimeContext, Animation, Model, BoneNameHash) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h +
lumix_compat_animator.h. Syntax-only, as tests/test_particle_system_compile.py: the engine itself cannot be linked here. The first is
skipped where the reference tree is absent."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_animator.h"\n'
       "bool use(Lumix::GpuAnimators& g, const Lumix::anim::RuntimeContext& ctx, Lumix::Animation* clip) {\n"
       "\tg.setAnimation(clip, 3u);\n"
       "\tg.begin();\n"
       "\tbool ok = g.add(ctx);\n"
       "\tg.addNone();\n"
       "\treturn ok && g.eval() && g.instructionCount() > 0 && g.lastError() != nullptr;\n"
       "}\n")


def test_animator_adapter_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "animator_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_animator_adapter_compiles_standalone(tmp_path):
    tu = tmp_path / "animator_tu.cpp"
    tu.write_text(USE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
