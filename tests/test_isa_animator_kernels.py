"""The kernels of animator_kernels.hip as the build compiles them for gfx950 (no GPU needed: hipcc -S).

Arithmetic: k_animators_update is compared bit for bit with the reference's FMA-free scalar fp32 and fp64 (animation/nodes.cpp), and
k_animators_root_motion with Transform arithmetic, so neither may hold a fused multiply-add of the algorithm's own; the compiler's
expansions of one IEEE division or square root are recognised by their opening instruction, as in tests/test_isa_no_fma.py. The
conversions to u32 are integer code (lmx_controller_program.h): no conversion expansion with an FMA either.

Residency: one lane per Animator. The VM's explicit stacks are indexed at run time and are scratch by design - the pose
frames (8 x 48 B), the value operands and the skip list: 400 bytes a lane in the first build, asserted here as a ceiling of 512. No LDS,
no atomics. The other three kernels are copies and one transform per lane: no scratch, no LDS."""
import re

from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick

SOURCE = "animator_kernels.hip"
OPENER = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")
KERNELS = ("k_animators_update", "k_animators_pack", "k_animators_set_inputs", "k_animators_root_motion")


def test_no_fused_multiply_add_outside_division_and_root(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    for tag in KERNELS:
        bodies = [b for name, b in ks.items() if tag in name]
        assert len(bodies) == 1, f"{tag} not in the ISA: {list(ks)}"
        body = bodies[0]
        bad = [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28): i])]
        assert not bad, f"{tag} contains fused multiply-adds of its own: {bad[:5]}"
    update = "\n".join(next(b for name, b in ks.items() if "k_animators_update" in name))
    # lerp / nlerp / rotate as separate products and sums, Time's arithmetic in fp64, nlerp's root and the IEEE divisions
    assert len(re.findall(r"\bv_(pk_)?mul_f32", update)) >= 30 and len(re.findall(r"\bv_(pk_)?(add|sub)_f32", update)) >= 30
    assert "v_sqrt_f32" in update and "v_div_fixup_f32" in update and "v_div_fixup_f64" in update and "v_cvt_f64_u32" in update
    assert "v_trunc_f32" in update, "fmodf(relt, 1) is x - trunc(x)"
    for text in ("\n".join(b) for b in ks.values()):
        assert not re.search(r"\b(ds_add|ds_cmpst|ds_max|ds_min|global_atomic|flat_atomic|buffer_atomic)", text), "no atomics"
        assert "buffer_wbl2" not in text and "buffer_inv" not in text, "no device-scope fence: launch boundaries order the hand-off"


def test_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    (up,) = pick(meta, "k_animators_update")
    assert up["group_segment_fixed_size"] == 0, up
    assert 0 < up["private_segment_fixed_size"] <= 512, f"scratch per lane: {up['private_segment_fixed_size']} B (first build: 400: the explicit stacks)"
    assert up["next_free_vgpr"] <= 192, f"{up['next_free_vgpr']} VGPRs (first build: 160)"
    for tag in KERNELS[1:]:
        (m,) = pick(meta, tag)
        assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, (tag, m)
        assert m["next_free_vgpr"] <= 64, (tag, m["next_free_vgpr"])
