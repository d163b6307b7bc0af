"""lumixengine_amd/host/gpu_draw_encoder.h - the engine-side walk over the LmxDrawRun records - against the reference's REAL headers
(DrawStream, gpu::Drawcall, Shader::getProgram, Model / Mesh / Material, RenderModule::getDecal) under -DLMX_WITH_LUMIX_HEADERS, and
standalone (the C-ABI half only). Syntax-only, as tests/test_plugin_compile.py: the engine itself cannot be linked here. Skipped where the
reference tree is absent."""
import os
import subprocess

import pytest

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture


def test_draw_encoder_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "draw_encoder_tu.cpp"
    tu.write_text('#include "gpu_draw_encoder.h"\n'
                  "void use(Lumix::GpuDrawEncoder& e, Lumix::RenderModule& m, const Lumix::GpuDrawEncoder::Bucket* b, const Lumix::GpuDrawEncoder::Shared& s) { e.encode(m, b, s); }\n")
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_draw_encoder_compiles_standalone():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-x", "c++", os.path.join(HOST, "gpu_draw_encoder.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
