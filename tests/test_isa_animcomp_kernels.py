"""animcomp_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: the tables and streams are compared byte for byte with tests/animcomp_oracle.py - fp32 differences and quotients, pack's fp64
divide, multiply and add of 0.5 as three operations - so no kernel may hold a fused multiply-add of the algorithm's own. The compiler's own:
the expansion of an IEEE division (recognised by its opening instruction, as in tests/test_isa_grass_kernels.py), of an unsigned integer
division (entry / tracks, thread / columns: by the constants only it uses, as in tests/test_isa_voxel_kernels.py), and of the conversion of
a double to 64 unsigned bits, which splits the truncated value with one v_fma_f64 by -2^32 (exact: it forms the low word's value).

Residency: no kernel uses scratch. k_animcomp_pack declares one group of 32 frames of the widest frame there is,
196 bones x 57 bits = 11 172 dwords, 44 688 bytes: three workgroups share a CU's 160 KiB, three waves per SIMD. The compiler knows that
and raises the kernel's register allocation to what three waves leave each other (it needs 42 and declares 129); up to 168 VGPRs three
waves still fit a SIMD's 512, so the LDS decides. k_animcomp_ranges declares 256 partial folds of 12 bytes, k_animcomp_layout the scan's four words
and the clip's code; at up to 64 VGPRs eight of their waves fit a SIMD."""
import re

from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick
from tests.test_isa_grass_kernels import OPENER
from tests.test_isa_voxel_kernels import INT_DIV

SOURCE = "animcomp_kernels.hip"
KERNELS = ("k_animcomp_ranges", "k_animcomp_layout", "k_animcomp_pack")
TO_U64 = re.compile(r"v_fma_f64.*0xc1f00000")  # (uint64_t)double: trunc, * 2^-32, floor, fma(floor, -2^32, trunc)


def stray_fma(body):
    return [l for i, l in enumerate(body) if FMA.search(l) and not INT_DIV.search(l) and not TO_U64.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28): i])]


def test_no_fused_multiply_add_outside_divisions_and_conversions(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    for tag in KERNELS:
        assert sum(tag in name for name in ks) == 1, f"{tag}: {list(ks)}"
    for name, body in ks.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    for name, body in ks.items():
        text = "\n".join(body)
        if "k_animcomp_pack" in name:
            assert "v_div_fixup_f64" in text and "v_mul_f64" in text and "v_add_f64" in text, "pack: an fp64 divide, an fp64 multiply, then the add of 0.5"
            assert sum("v_sub_f32" in l or "v_subrev_f32" in l or "v_pk_add_f32" in l or "v_add_f32" in l for l in body) >= 1, "v - min in fp32"
            assert re.search(r"ds_or_b32", text), "entries are set with LDS atomic ORs"
            assert not re.search(r"(global|flat)_atomic", text), "no global atomic touches a stream"
        if "k_animcomp_layout" in name:
            assert text.count("v_div_fixup_f32") >= 2, "range / step / error and range / (2^b - 1) are IEEE divisions"
        if "k_animcomp_ranges" in name:
            assert not re.search(r"v_(min|max)(_num)?_f32", text), "the fold is `p < min ? p : min`, not a min instruction (which would lose the sign of a zero)"


def test_animcomp_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        (k,) = pick(meta, tag)
        assert k["private_segment_fixed_size"] == 0, (tag, k)
        assert k["next_free_sgpr"] <= 104, k
    (k,) = pick(meta, "k_animcomp_pack")
    group = 196 * 57 * 4
    assert k["group_segment_fixed_size"] == group == 44688, k
    assert 160 * 1024 // group == 3, "three workgroups per CU"
    assert k["next_free_vgpr"] <= 168, f"{k['next_free_vgpr']} VGPRs: the registers, not the LDS, would set the residency"
    (k,) = pick(meta, "k_animcomp_ranges")
    assert k["group_segment_fixed_size"] == 256 * 12 and k["next_free_vgpr"] <= 64, k
    (k,) = pick(meta, "k_animcomp_layout")
    assert k["group_segment_fixed_size"] == 4 * 4 + 4 and k["next_free_vgpr"] <= 64, k
