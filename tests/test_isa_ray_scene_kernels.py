"""ray_scene_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S), held to what tests/test_isa_ray_kernels.py asks of
its siblings: the kernels exist, none spills, none holds a fused multiply-add of the algorithm's own (the expansions of one IEEE division
are recognised by their opening instruction), and the divisions - 1.0f / x of the slab test and of getHeight, start / scale, the `next`
and `delta` quotients of the walk, the triangle test's - are the correctly rounded sequence that ends in v_div_fixup_f32."""
from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_ray_kernels import OPENER
from tests.test_isa_residency import metadata

KERNELS = ("k_pgray_broad", "k_pgray_resolve", "k_pgray_write", "k_terrain_ray", "k_ray_scene_write")


def test_scene_ray_kernels_contain_no_fused_multiply_add(tmp_path):
    ks = kernels(isa_of("ray_scene_kernels.hip", tmp_path))
    for tag in KERNELS:
        bodies = [body for name, body in ks.items() if tag in name]
        assert len(bodies) == 1, f"{tag} not (once) in the ISA: {list(ks)}"
        body = bodies[0]
        bad = [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28) : i])]
        assert not bad, f"{tag} contains fused multiply-adds: {bad[:5]}"
    terrain = next(body for name, body in ks.items() if "k_terrain_ray" in name)
    assert sum("mul_f32" in l for l in terrain) >= 30  # the interpolation and the two triangle tests are there, as separate multiplies and adds


def test_divisions_are_correctly_rounded(tmp_path):
    ks = kernels(isa_of("ray_scene_kernels.hip", tmp_path))
    for tag, at_least in (("k_pgray_broad", 3), ("k_terrain_ray", 6), ("k_pgray_resolve", 1)):
        body = next(body for name, body in ks.items() if tag in name)
        count = lambda op: sum(op in l for l in body)
        assert count("v_div_fixup_f32") >= at_least and count("v_div_scale_f32") >= 1, f"{tag}: a division is not the IEEE one"
        # the expansion of one division holds one v_rcp_f32, one v_div_fmas_f32 and one v_div_fixup_f32: a bare reciprocal used as a
        # quotient would leave more reciprocals than fix-ups
        assert count("v_rcp_f32") == count("v_div_fmas_f32") == count("v_div_fixup_f32"), f"{tag}: v_rcp_f32 outside a division"


def test_scene_ray_kernels_use_no_scratch(tmp_path):
    meta = metadata("ray_scene_kernels.hip", tmp_path)
    for tag in KERNELS:
        hits = [v for k, v in meta.items() if tag in k]
        assert hits, f"no kernel matching {tag}"
        for k in hits:
            assert k["private_segment_fixed_size"] == 0, (tag, k)
