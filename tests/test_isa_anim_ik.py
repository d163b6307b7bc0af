"""k_anim_blend_instrs and k_anim_blend_stack as the build compiles them for gfx950 (no GPU needed: hipcc -S).

Arithmetic: both are compared bit for bit with the reference's FMA-free scalar fp32 (evalIK, Animation::getRelativePose), so neither may
hold a fused multiply-add of the algorithm's own; the compiler's expansions of one IEEE division or square root are recognised by their
opening instruction, as in tests/test_isa_no_fma.py.

Residency: one-wave blocks. k_anim_blend_instrs keeps the staged pose (196 bones x 28 B) and the chain arrays of evalIK in
static LDS - every chain array is indexed by run-time values, so a private array would be scratch: none is allowed. The figures are what
the first build showed: 8320 B of LDS (19 blocks per CU by LDS) and 86 VGPRs (<= 96: five waves per SIMD, 20 blocks per CU - LDS and
registers admit about the same). k_anim_blend_stack: 46 VGPRs, no LDS."""
import re

from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick

SOURCE = "anim_kernels.hip"
OPENER = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")


def test_no_fused_multiply_add_outside_division_and_root(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    for tag in ("k_anim_blend_instrs", "k_anim_blend_stack"):
        bodies = [b for name, b in ks.items() if tag in name]
        assert len(bodies) == 1, f"{tag} not in the ISA: {list(ks)}"
        body = bodies[0]
        bad = [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28): i])]
        assert not bad, f"{tag} contains fused multiply-adds of its own: {bad[:5]}"
        # the products and sums are there as separate (scalar or packed) instructions
        assert sum(bool(re.search(r"\bv_(pk_)?mul_f32", l)) for l in body) >= 10 and sum(bool(re.search(r"\bv_(pk_)?(add|sub)_f32", l)) for l in body) >= 10
    ik = next(b for name, b in ks.items() if "k_anim_blend_instrs" in name)
    # normalize / length / nlerp: 1 / sqrtf(..) as the correctly rounded root and the IEEE division
    text = "\n".join(ik)
    assert "v_sqrt_f32" in text and "v_div_fixup_f32" in text and "v_div_scale_f32" in text
    assert "v_sin_f32" not in text and "v_cos_f32" not in text, "Quat(n, PI) carries its two constants: no device sine or cosine"
    assert not re.search(r"\b(ds_add|ds_cmpst|ds_max|ds_min|global_atomic|flat_atomic|buffer_atomic)", text), "no atomics"
    assert "buffer_wbl2" not in text and "buffer_inv" not in text, "no device-scope fence: launch boundaries order it against lmx_skin_run"


def test_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    (ik,) = pick(meta, "k_anim_blend_instrs")
    assert ik["private_segment_fixed_size"] == 0, f"scratch: {ik}"  # the chain arrays live in LDS
    assert ik["group_segment_fixed_size"] == 8320, ik  # 196 x 12 + 196 x 16 (pose) + 2832 (IkChain)
    assert ik["next_free_vgpr"] <= 96, f"{ik['next_free_vgpr']} VGPRs: five one-wave blocks per SIMD need <= 96 (first build: 86)"
    (bs,) = pick(meta, "k_anim_blend_stack")
    assert bs["private_segment_fixed_size"] == 0 and bs["group_segment_fixed_size"] == 0, bs
    assert bs["next_free_vgpr"] <= 48, f"{bs['next_free_vgpr']} VGPRs (first build: 46)"
