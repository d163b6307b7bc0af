"""texmips_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: the chains are compared bit for bit with the FMA-free fp32 of tests/texmips_oracle.py (the taps' multiplies and adds, the
premultiplied channels, x * 255 + 0.5), so no kernel may hold a fused multiply-add of the algorithm's own. The compiler's expansion of an IEEE
division (1.0f / A, the coverage walk's quotients, the fp64 count / pixels) is recognised by its opening instruction, and that of the
generator's 64-bit modulo by its constants, as in tests/test_isa_voxel_kernels.py.

Residency (DESIGN.md §4.24's table): no kernel uses scratch - the taps are read from LDS where they are indexed at run time. The filtered
k_mip_level declares the 48 x 48 window (9216 bytes), seven planes of 48 x 16 floats (21 504), the taps of 16 columns and 16 rows (2048) and
the 256 alpha bins (1024): 33 792 bytes, and 2048 more for the two sRGB tables. Four workgroups share a CU's 160 KiB, four waves per SIMD,
and at up to 128 VGPRs the registers allow that too: the LDS decides. The stochastic form and k_mip_scale declare the 256 bins alone.
k_mip_tail declares two levels of at most 32 x 32 words (8192) and the bins, the filtered forms seven planes of 32 x 16 floats (14 336)
besides and the sRGB form its tables: 9216, 23 552 and 25 600 bytes, one workgroup per chain."""
from tests.test_isa_no_fma import isa_of, kernels
from tests.test_isa_residency import metadata, pick
from tests.test_isa_voxel_kernels import stray_fma

SOURCE = "texmips_kernels.hip"
KERNELS = ("k_mip_level", "k_mip_tail", "k_mip_scale", "k_mip_coverage")
LINEAR, SRGB, STOCHASTIC = "k_mip_levelILi0E", "k_mip_levelILi1E", "k_mip_levelILi2E"
TAIL_LINEAR, TAIL_SRGB, TAIL_STOCHASTIC = "k_mip_tailILi0E", "k_mip_tailILi1E", "k_mip_tailILi2E"


def test_no_fused_multiply_add_outside_divisions(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    assert sum("k_mip_level" in name for name in ks) == 3 and sum("k_mip_tail" in name for name in ks) == 3 and sum("k_mip_scale" in name for name in ks) == 1 and sum("k_mip_coverage" in name for name in ks) == 1, list(ks)
    for name, body in ks.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    for name, body in ks.items():
        text = "\n".join(body)
        if TAIL_LINEAR in name or TAIL_SRGB in name or TAIL_STOCHASTIC in name:
            assert "v_div_fixup_f64" in text and text.count("v_div_fixup_f32") >= 2, "the tail's own coverage walk: count / pixels in fp64, the walk's quotients in fp32"
        if TAIL_STOCHASTIC in name:
            assert "v_mul_f64" in text, "randFloat's product is not the fp64 one"
        if LINEAR in name or SRGB in name or TAIL_LINEAR in name or TAIL_SRGB in name:
            assert text.count("v_div_fixup_f32") >= 1, "1.0f / A is not an IEEE division"
            assert sum("mul_f32" in l for l in body) >= 8 and sum("add_f32" in l for l in body) >= 8, "the taps, as separate multiplies and adds (packed pairs included)"
            assert sum("ds_read" in l or "ds_load" in l for l in body) >= 4 and sum("ds_write" in l or "ds_store" in l for l in body) >= 8, "the window, the taps and the seven planes are in LDS"
        if STOCHASTIC in name:
            assert "v_mul_f64" in text, "randFloat's product is not the fp64 one"
            assert text.count("v_div_fixup_f32") >= 2, "w / float(dst_w) and h / float(dst_h) are not IEEE divisions"
        if "k_mip_scale" in name:
            assert "v_div_fixup_f64" in text and text.count("v_div_fixup_f32") >= 2, "count / pixels in fp64, the walk's quotients in fp32"


def test_texmips_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        for k in pick(meta, tag):
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    window, planes, taps, bins, tables = 48 * 48 * 4, 7 * 48 * 16 * 4, 2 * 16 * 64, 256 * 4, 512 * 4
    for tag, lds in ((LINEAR, window + planes + taps + bins), (SRGB, window + planes + taps + bins + tables)):
        (k,) = pick(meta, tag)
        assert k["group_segment_fixed_size"] == lds and lds in (33792, 35840), k
        assert 160 * 1024 // lds == 4, "four workgroups per CU"
        assert k["next_free_vgpr"] <= 128, f"{k['next_free_vgpr']} VGPRs: fewer than four waves per SIMD, the LDS no longer sets the residency"
        assert k["next_free_sgpr"] <= 104, k
    (k,) = pick(meta, STOCHASTIC)
    assert k["group_segment_fixed_size"] == bins and k["next_free_vgpr"] <= 32, k
    two_levels, tail_planes = 2 * 32 * 32 * 4, 7 * 32 * 16 * 4
    for tag, lds, vgprs in ((TAIL_LINEAR, two_levels + bins + tail_planes, 96), (TAIL_SRGB, two_levels + bins + tail_planes + tables, 96), (TAIL_STOCHASTIC, two_levels + bins, 48)):
        (k,) = pick(meta, tag)
        assert k["group_segment_fixed_size"] == lds and lds in (23552, 25600, 9216), k
        assert k["next_free_vgpr"] <= vgprs and k["next_free_sgpr"] <= 104, k
    (k,) = pick(meta, "k_mip_scale")
    assert k["group_segment_fixed_size"] == bins and k["next_free_vgpr"] <= 32, k
    (k,) = pick(meta, "k_mip_coverage")
    assert k["group_segment_fixed_size"] == 4 and k["next_free_vgpr"] <= 16, k
