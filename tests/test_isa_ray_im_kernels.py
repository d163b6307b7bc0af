"""The instanced-model kernels of ray_kernels.hip as the build compiles them for gfx950 (no GPU needed: hipcc -S), held to what
tests/test_isa_ray_kernels.py asks of their siblings: they exist, none spills, none holds a fused multiply-add of the algorithm's own (the
expansions of one IEEE division or square root are recognised by their opening instruction), and k_imray_broad's sqrtf - the w of an
instance's quaternion and the sphere test's root - and its 1 / scale are the correctly rounded forms."""
import re

from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_ray_kernels import OPENER
from tests.test_isa_residency import metadata

KERNELS = ("k_imray_broad", "k_imray_resolve", "k_imray_write")


def test_im_ray_kernels_contain_no_fused_multiply_add(tmp_path):
    ks = kernels(isa_of("ray_kernels.hip", tmp_path))
    for tag in KERNELS:
        bodies = [body for name, body in ks.items() if tag in name]
        assert len(bodies) == 1, f"{tag} not (once) in the ISA: {list(ks)}"
        body = bodies[0]
        bad = [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28) : i])]
        assert not bad, f"{tag} contains fused multiply-adds: {bad[:5]}"
    broad = next(body for name, body in ks.items() if "k_imray_broad" in name)
    assert sum("mul_f32" in l for l in broad) >= 30  # the sphere test and the two rotations are there, as separate multiplies and adds


def test_im_broad_roots_and_division_are_correctly_rounded(tmp_path):
    ks = kernels(isa_of("ray_kernels.hip", tmp_path))
    broad = next(body for name, body in ks.items() if "k_imray_broad" in name)
    text = "\n".join(broad)
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text, "1 / scale is not the IEEE division"
    roots = [i for i, l in enumerate(broad) if re.search(r"\bv_sqrt_f32", l)]
    assert len(roots) >= 2, "the quaternion's w and the sphere test each take a square root"
    for i in roots:  # the hardware's 1-ulp v_sqrt_f32 is followed by the compiler's fix-up (fma residuals + compares), never used alone
        assert any(FMA.search(p) for p in broad[i : i + 28]), "v_sqrt_f32 without the rounding fix-up behind it"


def test_im_ray_kernels_use_no_scratch(tmp_path):
    meta = metadata("ray_kernels.hip", tmp_path)
    for tag in KERNELS:
        hits = [v for k, v in meta.items() if tag in k]
        assert hits, f"no kernel matching {tag}"
        for k in hits:
            assert k["private_segment_fixed_size"] == 0, (tag, k)
