"""voxel_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: voxel bytes, AO floats and baked u8 values are compared bit for bit with the reference's FMA-free fp32, so none of the four
kernels may hold a fused multiply-add of the algorithm's own. The compiler's expansion of an IEEE division is recognised by its opening
instruction, as in tests/test_isa_grass_kernels.py; its expansion of a 64-bit integer division (a ray's voxel = ray / ray_count) by the
float constants 2^32, 2^-32 and their neighbours that only it uses.

Residency: no kernel uses scratch. k_voxel_ao<true> declares the bit mask - VOXEL_AO_LDS_WORDS words, 40 KiB - so four
256-lane blocks share a CU's 160 KiB, sixteen waves, four per SIMD; at up to 128 VGPRs the registers allow that too, so the LDS decides.
The global-memory form, k_voxel_raster, k_voxel_blur and k_voxel_sample declare no LDS."""
import re

from lumixengine_amd import api
from tests.test_isa_grass_kernels import OPENER
from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick

SOURCE = "voxel_kernels.hip"
KERNELS = ("k_voxel_raster", "k_voxel_ao", "k_voxel_blur", "k_voxel_sample")
INT_DIV = re.compile(r"0x4f800000|0x5f7ffffc|0x2f800000|0xcf800000|0x4f7ffffe")  # 2^32, 2^64 - ulp, 2^-32, -2^32, 2^32 - ulp


def stray_fma(body):
    return [l for i, l in enumerate(body) if FMA.search(l) and not INT_DIV.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28): i])]


def test_no_fused_multiply_add_outside_divisions(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in ks), f"{tag} not in the ISA: {list(ks)}"
    assert sum("k_voxel_ao" in name for name in ks) == 2, "the LDS and the global-memory form"
    for name, body in ks.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    for name, body in ks.items():
        text = "\n".join(body)
        if "k_voxel_ao" in name:
            assert "v_mul_f64" in text, "randFloat's product is not the fp64 one"
            assert "v_div_fixup_f32" in text, "1.0f / max and 1.f / ray_count are not IEEE divisions"
            assert sum("add_f32" in l for l in body) >= 5, "p += d is not made of separate adds (packed pairs included)"
        if "k_voxel_raster" in name:
            # the nine cross axes, the plane and the box's corners as separate multiplies and adds (packed pairs included)
            assert sum("mul_f32" in l for l in body) >= 20 and sum("sub_f32" in l or "add_f32" in l for l in body) >= 20
            assert re.search(r"\b(global|flat)_store_byte\b", text), "the voxel is not written with a byte store"
        if "k_voxel_blur" in name:
            assert sum("add_f32" in l for l in body) >= 27 and "v_div_fixup_f32" in text
        if "k_voxel_sample" in name:
            assert text.count("v_div_fixup_f32") >= 3, "(p - min) / (max - min) is not the IEEE division, per component"


def test_voxel_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        for k in pick(meta, tag):
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    lds = [k for name, k in meta.items() if "k_voxel_ao" in name and k["group_segment_fixed_size"]]
    glob = [k for name, k in meta.items() if "k_voxel_ao" in name and not k["group_segment_fixed_size"]]
    assert len(lds) == 1 and len(glob) == 1
    assert lds[0]["group_segment_fixed_size"] == 4 * api.VOXEL_AO_LDS_WORDS == 40960
    assert 160 * 1024 // lds[0]["group_segment_fixed_size"] == 4 and 32 * api.VOXEL_AO_LDS_WORDS >= 68 ** 3
    assert lds[0]["next_free_vgpr"] <= 128, f"{lds[0]['next_free_vgpr']} VGPRs: fewer than four waves per SIMD, the LDS no longer sets the residency"
    assert glob[0]["next_free_vgpr"] <= 64, glob[0]
    for tag, vgprs in (("k_voxel_raster", 128), ("k_voxel_blur", 64), ("k_voxel_sample", 64)):
        for k in pick(meta, tag):
            assert k["next_free_vgpr"] <= vgprs and k["group_segment_fixed_size"] == 0 and k["next_free_sgpr"] <= 104, (tag, k)
