"""cluster_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S): records and cluster ranges are compared bit for bit
with the reference's FMA-free scalar arithmetic (planeDist, color * intensity), so the file must not hold a single fused multiply-add;
and none of its kernels may spill - the planes arrive as a 2.3 KB kernel argument that the record step indexes per lane, which must
become loads from the argument segment, not a private copy."""
from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata

KERNELS = ("k_cluster_records", "k_cluster_gather", "k_cluster_offsets")


def test_cluster_kernels_contain_no_fused_multiply_add(tmp_path):
    ks = kernels(isa_of("cluster_kernels.hip", tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in ks), f"{tag} not in the ISA: {list(ks)}"
    assert sum("k_cluster_gather" in name for name in ks) == 2  # the count and the fill instance
    for name, body in ks.items():
        bad = [l for l in body if FMA.search(l)]
        assert not bad, f"{name} contains fused multiply-adds: {bad[:5]}"
    rec = next(body for name, body in ks.items() if "k_cluster_records" in name)
    assert sum("mul_f32" in l for l in rec) >= 9  # the plane distances are there, as separate multiplies and adds


def test_cluster_kernels_use_no_scratch(tmp_path):
    meta = metadata("cluster_kernels.hip", tmp_path)
    for tag in KERNELS:
        hits = [v for k, v in meta.items() if tag in k]
        assert hits, f"no kernel matching {tag}"
        for k in hits:
            assert k["private_segment_fixed_size"] == 0, (tag, k)
