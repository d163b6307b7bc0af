"""The ribbon kernels of particle_kernels.hip as the build compiles them for gfx950 (no GPU needed: hipcc -S).

Arithmetic: as for the other particle kernels (tests/test_isa_particle_kernels.py, whose helpers this file uses) - compiled with
-DLMX_PARTICLE_NO_LIBM no fused multiply-add may be left outside the expansions of one division, root or float -> i64 conversion.

Residency: k_particles_ribbon_chunk runs 1024-lane blocks of floor(1024 / max_ribbon_length) whole ribbons - 16 waves, four
per SIMD - whose VM registers are dynamic LDS pages of 4 KiB. Two blocks per CU need <= 64 VGPRs and no scratch, and static LDS stays 0 so
that 16 register pages fit twice into the CU's 160 KiB. k_particles_ribbon_emit runs 256-lane blocks with 16 KiB of static LDS (the emit
program's registers): ten blocks per CU by LDS; six waves per SIMD need <= 80 VGPRs."""
from tests.test_isa_no_fma import isa_of, kernels
from tests.test_isa_particle_kernels import SOURCE, isa_without_libm, stray_fma
from tests.test_isa_residency import metadata, pick

KERNELS = ("k_particles_ribbon_emit", "k_particles_ribbon_commit", "k_particles_ribbon_chunkILb0E", "k_particles_ribbon_chunkILb1E")


def test_no_fused_multiply_add_of_their_own(tmp_path):
    real = kernels(isa_of(SOURCE, tmp_path))
    bare = kernels(isa_without_libm(tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in real), f"{tag} not in the ISA: {list(real)}"
        bodies = [body for name, body in bare.items() if tag in name]
        assert bodies, f"{tag} not in the ISA without libm: {list(bare)}"
        for body in bodies:
            assert len(body) > 8, f"{tag}: the listing ends at an early exit ({len(body)} instructions)"
            bad = stray_fma(body)
            assert not bad, f"{tag} contains fused multiply-adds of its own: {bad[:5]}"


def test_ribbon_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        found = pick(meta, tag)
        assert found, tag
        for k in found:
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    for tag in ("k_particles_ribbon_chunkILb0E", "k_particles_ribbon_chunkILb1E"):
        for k in pick(meta, tag):
            assert k["next_free_vgpr"] <= 64, f"{tag}: {k['next_free_vgpr']} VGPRs - two 16-wave blocks per CU need <= 64"
            assert k["next_free_sgpr"] <= 104, (tag, k)
            assert k["group_segment_fixed_size"] == 0, (tag, k)  # the register pages are the launch's dynamic LDS
    for k in pick(meta, "k_particles_ribbon_emit"):
        assert k["next_free_vgpr"] <= 80 and k["group_segment_fixed_size"] == 16 * 256 * 4, k
