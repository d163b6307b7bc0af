"""texcomp_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: the blocks are compared bit for bit with the FMA-free fp32 of tests/texcomp_oracle.py (the least-squares solve, the selector
projection of check 2, the power iteration), so no kernel may hold a fused multiply-add of the algorithm's own. The compiler's expansion of
an IEEE division is recognised by its opening instruction, as in tests/test_isa_voxel_kernels.py.

Residency (DESIGN.md §4.23's table): no kernel uses scratch - the sixteen pixels, the palette and the selectors are never indexed at run
time. k_bc1_search declares the staged tables, (969 + 153) x 16 bytes of histograms and 96 midpoints: 18 336 bytes, so LDS admits eight
workgroups per CU and the registers set the residency: both instantiations are held to 128 VGPRs, four waves per SIMD, so that the largest
grid (1024 workgroups of four waves) is resident at once. k_bc4 declares no LDS."""
from tests.test_isa_no_fma import isa_of, kernels
from tests.test_isa_residency import metadata, pick
from tests.test_isa_voxel_kernels import stray_fma

SOURCE = "texcomp_kernels.hip"
KERNELS = ("k_bc4", "k_bc1_search")


def test_no_fused_multiply_add_outside_divisions(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    assert sum("k_bc4" in name for name in ks) == 1 and sum("k_bc1_search" in name for name in ks) == 2, list(ks)  # with and without 3-colour blocks
    for name, body in ks.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    for name, body in ks.items():
        text = "\n".join(body)
        if "k_bc1_search" in name:
            assert text.count("v_div_fixup_f32") >= 2, "4.0f / (...) of check 2 and 2048.0f / k are not IEEE divisions"
            assert sum("mul_f32" in l for l in body) >= 12 and sum("add_f32" in l for l in body) >= 6, "the 2 x 2 solve per channel, as separate multiplies and adds"
            assert sum("ds_read" in l or "ds_load" in l for l in body) >= 1, "the histograms come from LDS"
            assert sum("ds_bpermute" in l for l in body) >= 4, "a trial reads the prefix sums of other lanes"


def test_texcomp_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        for k in pick(meta, tag):
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    search = pick(meta, "k_bc1_search")
    assert len(search) == 2
    for k in search:
        assert k["group_segment_fixed_size"] == ((969 + 153) * 4 + 96) * 4 == 18336, k
        assert k["next_free_vgpr"] <= 128, f"{k['next_free_vgpr']} VGPRs: fewer than four waves per SIMD, the largest grid is no longer resident at once"
        assert k["next_free_sgpr"] <= 104, k
    bc4 = pick(meta, "k_bc4")[0]
    assert bc4["group_segment_fixed_size"] == 0 and bc4["next_free_vgpr"] <= 48, bc4
