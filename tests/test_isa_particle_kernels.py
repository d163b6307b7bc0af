"""particle_kernels.hip as the build compiles it for gfx950 (no GPU needed: hipcc -S).

Arithmetic: the VM's results are compared bit for bit with the reference's FMA-free fp32, so no kernel of the file may hold a fused
multiply-add of the algorithm's own. The compiler's expansions of one IEEE division or square root are recognised by their opening
instruction, as in tests/test_isa_no_fma.py; the library's fmod, sine and cosine are long expansions of their own, so the file is compiled
a second time with -DLMX_PARTICLE_NO_LIBM (those three calls replaced by plain arithmetic): what is left must hold no fused multiply-add
outside divisions and roots - every one of the real build therefore belongs to fmod, sine or cosine.

Residency: k_particles_chunk runs 1024-lane blocks - 16 waves, four per SIMD - whose VM registers are dynamic LDS pages of
4 KiB each. Two blocks per CU (8 waves per SIMD) need <= 64 VGPRs and no scratch; static LDS stays 0 so that 16 register pages and their
bookkeeping fit twice into the CU's 160 KiB. The decoded program comes through scalar loads."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_isa_no_fma import CSRC, FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick

SOURCE = "particle_kernels.hip"
KERNELS = ("k_particles_emit", "k_particles_commit", "k_particles_chunkILb0E", "k_particles_chunkILb1E", "k_particles_plan", "k_particles_compact", "k_particles_subemit", "k_particles_slices")
OPENER = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")
# gnoise's u32(floor(p)) goes through a 64-bit integer: the compiler's float -> i64 conversion (a multiply of |x| by 2^-32, v_floor and, right behind it,
# one fma by -2^32 that is exact) is an expansion of one source operation as well
TO_I64 = re.compile(r"\bv_floor_f32")


def isa_without_libm(tmp):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from lumixengine_amd import build as B

    out = tmp / "particle_kernels_no_libm.s"
    flags = [f for f in B.FLAGS if f not in ("-c", "-fPIC")] + ["-DLMX_PARTICLE_NO_LIBM=1"]
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-x", "hip", "-o", str(out), os.path.join(CSRC, SOURCE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text().splitlines()


def stray_fma(body):
    return [l for i, l in enumerate(body) if FMA.search(l) and not any(OPENER.search(p) for p in body[max(0, i - 28): i]) and not any(TO_I64.search(p) for p in body[max(0, i - 2): i])]


def test_no_fused_multiply_add_outside_division_root_sine_cosine_and_fmod(tmp_path):
    real = kernels(isa_of(SOURCE, tmp_path))
    bare = kernels(isa_without_libm(tmp_path))
    for tag in KERNELS:
        assert any(tag in name for name in real), f"{tag} not in the ISA: {list(real)}"
        assert any(tag in name for name in bare), f"{tag} not in the ISA without libm: {list(bare)}"
    for name, body in bare.items():
        bad = stray_fma(body)
        assert not bad, f"{name} contains fused multiply-adds of its own: {bad[:5]}"
    chunk = next(body for name, body in real.items() if "k_particles_chunkILb0E" in name)
    # MULTIPLY_ADD, MIX and gnoise are there as separate multiplies and adds; the division is the IEEE one
    text = "\n".join(chunk)
    assert sum("v_mul_f32" in l for l in chunk) >= 20 and sum("v_add_f32" in l or "v_sub_f32" in l for l in chunk) >= 20
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text, "a / b is not the IEEE division"
    for i, l in enumerate(chunk):
        if re.search(r"\bv_sqrt_f32", l):
            assert any(FMA.search(p) for p in chunk[i: i + 28]), "v_sqrt_f32 without the rounding fix-up behind it"


def test_particle_kernels_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    for tag in KERNELS:
        for k in pick(meta, tag):
            assert k["private_segment_fixed_size"] == 0, (tag, k)
    for tag in ("k_particles_chunkILb0E", "k_particles_chunkILb1E"):
        for k in pick(meta, tag):
            assert k["next_free_vgpr"] <= 64, f"{tag}: {k['next_free_vgpr']} VGPRs - two 16-wave blocks per CU need <= 64"
            assert k["next_free_sgpr"] <= 104, (tag, k)
            assert k["group_segment_fixed_size"] == 0, (tag, k)  # the register pages are the launch's dynamic LDS
    for k in pick(meta, "k_particles_emit"):  # 256-lane blocks, 16 registers x 256 lanes of LDS: nine blocks per CU by LDS, <= 56 VGPRs for nine waves per SIMD
        assert k["next_free_vgpr"] <= 56 and k["group_segment_fixed_size"] == 16 * 256 * 4, k


def test_the_program_comes_through_scalar_loads(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    for tag in ("k_particles_chunkILb0E", "k_particles_chunkILb1E"):
        body = next(b for name, b in ks.items() if tag in name)
        wide = [l for l in body if re.search(r"\bs_load_dwordx(2|4|8|16)\b", l)]
        assert len(wide) >= 6, f"{tag}: the decoded records are not read with scalar loads ({len(wide)} wide scalar loads)"
