"""Instanced models without a GPU: the scene reader's instanced-model section, the oracle's grid build on the demo map, the new PODs' layouts
against the C compiler, the adapter header against the reference's real headers and standalone, and the kernels' ISA (FMA-free, no scratch)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import im_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo_maps", "instanced_models.unv")
HOST = os.path.join(ROOT, "lumixengine_amd", "host")


@pytest.fixture(scope="module")
def api():
    from lumixengine_amd import api as a
    from lumixengine_amd import build

    if not os.path.exists(a.LIB_PATH):
        build.build()
    return a


def test_blob_reads_the_demo_maps_instanced_models(api):
    models = api.render_blob_read_instanced_models(open(DEMO, "rb").read())
    assert [(m["entity"], m["path"], len(m["instances"])) for m in models] == [(1, "engine/models/cube.fbx", 6), (2, "engine/models/sphere.fbx", 8)]
    for m in models:
        assert np.all(np.isfinite(m["instances"]["pos"])) and np.all(m["instances"]["scale"] > 0)
    # every other demo map has none
    other = api.render_blob_read_instanced_models(open(os.path.join(ROOT, "tests", "golden", "demo_maps", "demo.unv"), "rb").read())
    assert other == []


def test_blob_reader_reports_capacities(api):
    import ctypes as C

    lib = api.load_library()
    buf = np.frombuffer(open(DEMO, "rb").read(), np.uint8)
    nm, ni, npath = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib.lmx_render_blob_read_instanced_models(buf.ctypes.data_as(C.c_void_p), len(buf), 0, None, 0, None, 0, None, C.byref(nm), C.byref(ni), C.byref(npath))
    assert rc == 5 and (nm.value, ni.value) == (2, 14) and npath.value == len("engine/models/cube.fbx") + len("engine/models/sphere.fbx") + 2


def test_oracle_grid_build_is_idempotent_on_the_demo_map(api):
    """The file holds the instances in the order initInstancedModelGPUData left them: building the grid again keeps that order."""
    for m in api.render_blob_read_instanced_models(open(DEMO, "rb").read()):
        sorted_inst, g = O.grid_build(m["instances"])
        assert sorted_inst.tobytes() == np.ascontiguousarray(m["instances"]).tobytes()
        assert g["placed"] == len(m["instances"]) and g["unplaced"] == 0
        again, g2 = O.grid_build(sorted_inst)
        assert again.tobytes() == sorted_inst.tobytes() and np.array_equal(g["count"], g2["count"])


def test_oracle_grid_semantics():
    """A NaN coordinate never widens the grid and fails none of AABB::contains' tests: an all-NaN point lies in the first cell, a point
    with one NaN coordinate in the first cell its other coordinates fit. Large coordinates can leave rounding gaps between the cells."""
    inst = np.zeros(6, O.IM_INSTANCE)
    inst["pos"] = [[0, 0, 0], [10, 1, 10], [np.nan, 0, 5], [5, 0, 5], [9.99, 0.5, 0.01], [np.nan, np.nan, np.nan]]
    s, g = O.grid_build(inst)
    assert list(g["min"]) == [0, 0, 0] and list(g["max"]) == [10, 1, 10]
    assert g["placed"] == 6 and g["unplaced"] == 0
    assert np.all(np.isnan(s["pos"][1])) and g["count"][0] == 2  # cell 0: (0, 0, 0) and the all-NaN point, in input order
    assert np.isnan(s["pos"][g["from"][4], 0])  # (NaN, 0, 5): cell 4 (x fails no test, z = 5 lies in [2.49, 5.01])
    rng = np.random.default_rng(4)
    big = np.zeros(20000, O.IM_INSTANCE)
    big["pos"][:, 0] = (3.0e6 + rng.uniform(0, 2.7e3, len(big))).astype(np.float32)
    big["pos"][:, 2] = (-7.1e6 + rng.uniform(0, 3.3e3, len(big))).astype(np.float32)
    _, g = O.grid_build(big)
    assert g["placed"] + g["unplaced"] == len(big)


def test_oracle_runs_ten_million_instances_in_seconds():
    import time

    rng = np.random.default_rng(0)
    n = 10_000_000
    inst = np.zeros(n, O.IM_INSTANCE)
    inst["pos"][:, 0] = rng.uniform(-500, 500, n)
    inst["pos"][:, 2] = rng.uniform(-500, 500, n)
    inst["scale"] = 1
    from lumixengine_amd import api as a

    t = time.perf_counter()
    orc = O.Oracle()
    orc.set_model(0, [400, 3600, 22500, 90000], [(0, 0), (1, 1), (2, 2), (3, 3), (0, -1)], 1.0, [24, 18, 12, 6])
    orc.set_instances(0, inst)
    fr = a.frustum_perspective((0, 8, 0), np.array([0.3, -0.1, -1], np.float32), np.array([0, 1, 0], np.float32), 1.2, 1.7, 0.1, 2000.0)
    counts, recs, ind = orc.run(a.im_view((0, 8, 0)), fr)
    assert time.perf_counter() - t < 60 and len(recs) > 0 and len(ind) == 4


def test_struct_layouts_match_the_c_header(api, tmp_path):
    structs = {
        "LmxImInstance": (api.IM_INSTANCE, ["rot", "lod", "pos", "scale"]),
        "LmxBlobInstancedModel": (api.BLOB_INSTANCED_MODEL, ["entity", "path_offset", "first_instance", "instance_count"]),
        "LmxImCell": (api.IM_CELL, ["min", "max", "from_instance", "instance_count"]),
        "LmxImGrid": (api.IM_GRID, ["min", "max", "placed", "unplaced", "cells"]),
        "LmxImView": (api.IM_VIEW, ["camera_pos", "lod_multiplier", "time_delta", "is_shadow"]),
        "LmxImIndirect": (api.IM_INDIRECT, ["vertex_count", "instance_count", "first_index", "base_vertex", "base_instance"]),
        "LmxImCounts": (api.IM_COUNTS, ["bin_count", "bin_offset", "indirect_offset", "mesh_count", "instances", "unplaced"]),
    }
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lumix_mi355.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        for f in fields:
            lines.append(f'printf(" %zu", offsetof({name}, {f}));')
        lines.append('printf("\\n");')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out}
    for name, (dtype, fields) in structs.items():
        assert got[name] == [dtype.itemsize] + [dtype.fields[f][1] for f in fields], name
    assert got["LmxImInstance"][0] == 32 and got["LmxImIndirect"][0] == 20


def test_adapter_compiles_standalone():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-x", "c++",
                        os.path.join(HOST, "gpu_instanced_models.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_adapter_compiles_against_reference_headers(tmp_path):
    """GpuInstancedModels under -DLMX_WITH_LUMIX_HEADERS: InstancedModel / Model / World / ShiftedFrustum of the real headers, and the
    static_asserts that InstanceData is LmxImInstance byte for byte (same preparation as tests/test_plugin_compile.py)."""
    import shutil

    ref = "/root/reference"
    if not os.path.isdir(os.path.join(ref, "src")):
        pytest.skip("no reference tree on this machine")
    dst = tmp_path / "src"
    shutil.copytree(os.path.join(ref, "src"), dst)
    sync = dst / "core" / "sync.h"
    sync.write_text(sync.read_text().replace('#error "Not implemented"', "pthread_rwlock_t lock;", 1))
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "gpu_instanced_models.h"\n')
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-fno-exceptions", "-fno-rtti", "-DNDEBUG", "-DLMX_WITH_LUMIX_HEADERS", "-Wno-multichar", "-Wall", "-I" + str(dst),
           "-I" + os.path.join(ref, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _isa(tmp_path):
    import shutil

    from lumixengine_amd import build as B

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "im.s"
    flags = [f for f in B.FLAGS if f not in ("-c", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-x", "hip", "-o", str(out), os.path.join(ROOT, "lumixengine_amd", "csrc", "im_kernels.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


def test_kernels_are_fma_free_and_use_no_scratch(tmp_path):
    from tests.test_isa_no_fma import FMA, kernels

    text = _isa(tmp_path)
    ks = kernels(text.splitlines())
    names = [n for n in ks if any(t in n for t in ("k_im_grid_build", "k_im_count", "k_im_emit"))]
    assert len(names) == 3, list(ks)
    opener = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")
    for name in names:
        body = ks[name]
        bad = [l for i, l in enumerate(body) if FMA.search(l) and not any(opener.search(p) for p in body[max(0, i - 28) : i])]
        assert not bad, f"{name}: {bad[:5]}"
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", text):
        assert int(m.group(1)) == 0, "a kernel of im_kernels.hip spills to scratch"
    assert re.search(r"\.private_segment_fixed_size", text)
