"""pose_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S): the dual quaternions are compared bit for bit with the
reference's FMA-free scalar arithmetic, so the file must not hold a single fused multiply-add; and none of its kernels may spill."""
from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata

KERNELS = ("k_pose_sizes", "k_pose_offsets", "k_pose_dual_quats")


def test_pose_kernels_contain_no_fused_multiply_add(tmp_path):
    ks = kernels(isa_of("pose_kernels.hip", tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in ks), f"{tag} not in the ISA: {list(ks)}"
    for name, body in ks.items():  # every kernel of the file; none of them divides or takes a root, so no expansion may bring one in either
        bad = [l for l in body if FMA.search(l)]
        assert not bad, f"{name} contains fused multiply-adds: {bad[:5]}"
    dq = next(body for name, body in ks.items() if "k_pose_dual_quats" in name)
    assert sum("mul_f32" in l for l in dq) >= 10  # the arithmetic is there, as separate (scalar or packed) multiplies and adds


def test_pose_kernels_use_no_scratch(tmp_path):
    meta = metadata("pose_kernels.hip", tmp_path)
    for tag in KERNELS:
        hits = [v for k, v in meta.items() if tag in k]
        assert hits, f"no kernel matching {tag}"
        for k in hits:
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    # one wave per instance keeps 8 waves per SIMD resident (<= 64 VGPRs): the kernel hides its dependent loads with occupancy
    dq = [v for k, v in meta.items() if "k_pose_dual_quats" in k][0]
    assert dq["next_free_vgpr"] <= 64, dq
