"""probe_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: SH coefficients, mip texels, sampler results and RGBM bytes are compared bit for bit with FMA-free fp32, so none of the
kernels may hold a fused multiply-add of the algorithm's own - k_probe_filter included: what it adds to the sampler is held to a bound,
but the sampler inside it is the bit-exact one. The compiler's expansion of an IEEE division or square root is recognised by its opening
instruction, as in tests/test_isa_voxel_kernels.py.

Residency (DESIGN.md §4.22's table): no kernel uses scratch. k_sh_accumulate declares SH_CHUNK rows of SH_STRIDE floats and the
weight sum's word, 29 700 bytes: five 256-lane blocks share a CU's 160 KiB, and at up to 96 VGPRs the registers allow that too.
k_probe_filter declares the level's sample table, 128 x 3 floats; the other kernels declare no LDS."""
from lumixengine_amd import api
from tests.test_isa_no_fma import isa_of, kernels
from tests.test_isa_residency import metadata, pick
from tests.test_isa_voxel_kernels import stray_fma

SOURCE = "probe_kernels.hip"
KERNELS = ("k_sh_table", "k_sh_accumulate", "k_probe_mip", "k_probe_level0", "k_probe_filter", "k_probe_rgbm", "k_probe_sample")


def test_no_fused_multiply_add_outside_divisions_and_roots(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    for tag in KERNELS:
        assert sum(tag in name for name in ks) == 1, f"{tag}: {list(ks)}"
    for name, body in ks.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    for name, body in ks.items():
        text = "\n".join(body)
        if "k_sh_table" in name:
            assert text.count("v_div_fixup_f32") >= 4, "(x + 0.5f) / w, 4.0f / (...) and 1 / sqrtf are not IEEE divisions"
            assert "v_sqrt_f32" in text
        if "k_sh_accumulate" in name:
            # 27 products b * (c * w) per pixel (3 + 27 multiplies, packed pairs included), the chain as separate adds
            assert sum("mul_f32" in l for l in body) >= 15 and sum("add_f32" in l for l in body) >= 1
            assert sum("ds_write" in l or "ds_store" in l for l in body) >= 1 and sum("ds_read" in l or "ds_load" in l for l in body) >= 1
            assert "v_div_fixup_f32" in text, "(4.0f * PI) / weightSum is not the IEEE division"
        if "k_probe_mip" in name:
            assert sum("add_f32" in l for l in body) >= 6 and sum("mul_f32" in l for l in body) >= 2, "the sum of four and the 0.25f (packed pairs included)"
        if "k_probe_rgbm" in name:
            assert text.count("v_div_fixup_f32") >= 3, "x / m is not the IEEE division, per channel"
        if "k_probe_filter" in name:
            assert "v_log_f32" in text and sum("ds_read" in l or "ds_load" in l for l in body) >= 1


def test_probe_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        for k in pick(meta, tag):
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    acc = pick(meta, "k_sh_accumulate")[0]
    assert acc["group_segment_fixed_size"] == 4 * api.SH_CHUNK * api.SH_STRIDE + 4 == 29700
    assert 160 * 1024 // acc["group_segment_fixed_size"] == 5 and api.SH_STRIDE % 2 == 1 and api.SH_STRIDE >= 28 and api.SH_CHUNK == api.PROBE_BLOCK
    assert acc["next_free_vgpr"] <= 96, f"{acc['next_free_vgpr']} VGPRs: fewer than five blocks per CU, the LDS no longer sets the residency"
    flt = pick(meta, "k_probe_filter")[0]
    assert flt["group_segment_fixed_size"] == 128 * 3 * 4 and flt["next_free_vgpr"] <= 96, flt
    for tag, vgprs in (("k_sh_table", 32), ("k_probe_mip", 32), ("k_probe_level0", 64), ("k_probe_rgbm", 32), ("k_probe_sample", 64)):
        for k in pick(meta, tag):
            assert k["next_free_vgpr"] <= vgprs and k["group_segment_fixed_size"] == 0 and k["next_free_sgpr"] <= 104, (tag, k)
