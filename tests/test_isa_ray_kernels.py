"""ray_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S): hits are compared bit for bit with the reference's
FMA-free scalar arithmetic, so no kernel of the file may hold a fused multiply-add of the algorithm's own (the compiler's expansions of
one IEEE division or square root are recognised by their opening instruction, as in tests/test_isa_no_fma.py); none may spill (the narrow
phase blends twelve matrix elements per corner out of LDS); and 1.0f / x, sqrtf and the fp64 sqrt must be the correctly rounded forms -
their expansions end in v_div_fixup / carry the Newton steps, a bare v_rcp_f32 / v_sqrt_f32 result used as it is would not."""
import re

from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata

KERNELS = ("k_ray_broad", "k_ray_narrow", "k_ray_resolve", "k_ray_write")
OPENER = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")


def test_ray_kernels_contain_no_fused_multiply_add(tmp_path):
    ks = kernels(isa_of("ray_kernels.hip", tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in ks), f"{tag} not in the ISA: {list(ks)}"
    for name, body in ks.items():
        bad = [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28) : i])]
        assert not bad, f"{name} contains fused multiply-adds: {bad[:5]}"
    narrow = next(body for name, body in ks.items() if "k_ray_narrow" in name)
    assert sum("mul_f32" in l for l in narrow) >= 30  # the blend and the triangle test are there, as separate multiplies and adds


def test_divisions_and_roots_are_correctly_rounded(tmp_path):
    ks = kernels(isa_of("ray_kernels.hip", tmp_path))
    broad = next(body for name, body in ks.items() if "k_ray_broad" in name)
    text = "\n".join(broad)
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text, "1.0f / x is not the IEEE division"
    assert "v_div_fixup_f64" in text or "v_rsq_f64" in text or "v_sqrt_f64" in text, "no fp64 square root in the distance gate"
    # correctly rounded sqrtf: the hardware's 1-ulp v_sqrt_f32 is followed by the compiler's fix-up (fma residuals + compares), never used alone
    for i, l in enumerate(broad):
        if re.search(r"\bv_sqrt_f32", l):
            assert any(FMA.search(p) for p in broad[i : i + 28]), "v_sqrt_f32 without the rounding fix-up behind it"


def test_ray_kernels_use_no_scratch(tmp_path):
    meta = metadata("ray_kernels.hip", tmp_path)
    for tag in KERNELS:
        hits = [v for k, v in meta.items() if tag in k]
        assert hits, f"no kernel matching {tag}"
        for k in hits:
            assert k["private_segment_fixed_size"] == 0, (tag, k)
