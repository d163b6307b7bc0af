"""grass_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: positions, scales, AABBs, distances and counts are compared bit for bit with the reference's FMA-free fp32, so neither kernel
may hold a fused multiply-add of the algorithm's own. The compiler's expansions of one IEEE division or square root are recognised by
their opening instruction, as in tests/test_isa_particle_kernels.py, and so is its float -> 64-bit integer conversion (u32_of's slow path:
v_trunc_f32 and, right behind it, exact fused steps); the library's sine and cosine are long expansions of their own, so the file is compiled
a second time with -DLMX_GRASS_NO_LIBM (those two calls replaced by plain arithmetic): what is left must hold no fused multiply-add
outside divisions, roots and conversions - every other one of the real build therefore belongs to sinf or cosf.

Residency: k_grass_quads runs one-wave blocks whose static LDS - the 64 x 64 window, the list of 1024 accepted samples and
the count - allows seven blocks per CU of 160 KiB; up to 256 VGPRs leave two waves per SIMD, eight per CU, so the LDS decides. No scratch."""
import os
import re
import shutil
import subprocess

import pytest

from lumixengine_amd import api
from tests.test_isa_no_fma import CSRC, FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick

SOURCE = "grass_kernels.hip"
KERNELS = ("k_grass_quads", "k_grass_cull")
OPENER = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")
TO_I64 = re.compile(r"\bv_(floor|trunc)_f32")


def isa_without_libm(tmp):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from lumixengine_amd import build as B

    out = tmp / "grass_kernels_no_libm.s"
    flags = [f for f in B.FLAGS if f not in ("-c", "-fPIC")] + ["-DLMX_GRASS_NO_LIBM=1"]
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-x", "hip", "-o", str(out), os.path.join(CSRC, SOURCE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text().splitlines()


def stray_fma(body):
    return [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28): i]) and not any(TO_I64.search(p) for p in body[max(0, i - 4): i])]


def test_no_fused_multiply_add_outside_division_root_sine_and_cosine(tmp_path):
    real = kernels(isa_of(SOURCE, tmp_path))
    bare = kernels(isa_without_libm(tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in real), f"{tag} not in the ISA: {list(real)}"
        assert any(tag in name for name in bare), f"{tag} not in the ISA without libm: {list(bare)}"
    for name, body in bare.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    quads = next(body for name, body in real.items() if "k_grass_quads" in name)
    text = "\n".join(quads)
    # from + pn * quad_size and the height's interpolation are there as separate multiplies and adds; p / scale.x is the IEEE division
    assert sum("v_mul_f32" in l for l in quads) >= 10 and sum("v_add_f32" in l or "v_sub_f32" in l for l in quads) >= 10
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text, "p.x / m_scale.x is not the IEEE division"
    assert "v_mul_f64" in text, "randFloat's product is not the fp64 one"
    cull = next(body for name, body in real.items() if "k_grass_cull" in name)
    for i, l in enumerate(cull):
        if re.search(r"\bv_sqrt_f32", l):
            assert any(FMA.search(p) for p in cull[i: i + 28]), "v_sqrt_f32 without the rounding fix-up behind it"
    assert "v_div_fixup_f32" in "\n".join(cull)


def test_grass_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        for k in pick(meta, tag):
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    for k in pick(meta, "k_grass_quads"):
        # the window's bytes, 16 bytes per list entry, the count
        assert k["group_segment_fixed_size"] == api.GRASS_WINDOW * api.GRASS_WINDOW + 16 * api.GRASS_SAMPLES + 4, k
        assert 160 * 1024 // k["group_segment_fixed_size"] == 7
        assert k["next_free_vgpr"] <= 256, f"{k['next_free_vgpr']} VGPRs: fewer than two waves per SIMD, the LDS no longer sets the residency"
        assert k["next_free_sgpr"] <= 104, k
    for k in pick(meta, "k_grass_cull"):  # 256-lane blocks, one per view: far from any limit
        assert k["next_free_vgpr"] <= 128 and k["group_segment_fixed_size"] <= 256, k


def test_records_are_written_with_16_byte_stores(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    body = next(b for name, b in ks.items() if "k_grass_quads" in name)
    assert sum(1 for l in body if re.search(r"\b(global|flat)_store_dwordx4\b", l)) >= 4, "the two copies of a record are four 16-byte stores"
