"""GpuTextureCompressor::compressWithMips (lumixengine_amd/host/gpu_texture_compressor.h) RUN: tests/cpp/run_texture_mips.cpp fills the
Input- and stream-shaped mocks of tests/cpp/lumix_compat_texcomp.h and the Options shape of tests/cpp/lumix_compat_texmips.h from the cases
written here and calls compressWithMips(), as tests/test_gpu_adapters_texcomp.py does for compress(). Checked: the LBCHeader's bytes with the
generated `mips`; the payload's order for 2 slices and for 6 faces (chains in slice, face order, each level 0 .. behind the other); the RGBA8
case (6 x 4) as the chains' pixels; each of the three option combinations (stochastic, sRGB, linear) against tests/texmips_oracle.py, with
and without coverage scaling; refusals leaving the stream alone; and compress() still returning false for generate_mipmaps."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import texcomp_oracle as TO
from tests import texmips_oracle as MO
from tests.adapters_run import BUILD, CPP, HOST, ROOT, Out, library, u32

pytestmark = pytest.mark.gpu
NORMALMAP, ALPHA, CUBEMAP, COMPRESS, GENERATE_MIPMAPS, DROP_LAST_IMAGE, SRGB, STOCHASTIC = 1, 2, 4, 8, 16, 32, 64, 128
RGBA8, BC1, BC3, BC5 = 4, 15, 17, 19  # gpu::TextureFormat
LEAD = bytes([1, 2, 3])  # what the driver's stream holds before the adapter appends


def build_driver():
    """tests/cpp/run_texture_mips.cpp -> tests/_build/run_texture_mips (the recipe of tests/adapters_run.build_exe)"""
    library()
    src, exe = os.path.join(CPP, "run_texture_mips.cpp"), os.path.join(BUILD, "run_texture_mips")
    os.makedirs(BUILD, exist_ok=True)
    deps = [src, os.path.join(HOST, "gpu_texture_compressor.h")] + [os.path.join(CPP, h) for h in ("adapter_run.h", "lumix_compat.h", "lumix_compat_texcomp.h", "lumix_compat_texmips.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("lumix_mi355.h", "lmx_types.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    lib_dir = os.path.join(ROOT, "lumixengine_amd")
    tmp = f"{exe}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-multichar", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + CPP, src, "-o", tmp, "-L" + lib_dir, "-llumix_mi355",
                    "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    os.replace(tmp, exe)
    return exe


def case(rng, w, h, slices, flags, ref_norm=-0.5, mips=1, want=True):
    """-> (scenario bytes, the level-0 images in slice, face order uint8 (n, h, w, 4)); the scenario lists them in face, slice order"""
    faces = 6 if flags & CUBEMAP else 1
    blob = u32(w, h, slices, mips, flags, int(want)) + struct.pack("<f", ref_norm)
    images = rng.integers(0, 256, (mips, slices, faces, h, w, 4)).astype(np.uint8)
    for mip in range(mips):
        for f in range(faces):
            for s in range(slices):
                blob += images[mip, s, f, : max(h >> mip, 1), : max(w >> mip, 1)].tobytes()
    return blob, images[0].reshape(slices * faces, h, w, 4)


def run(tmp_path, scenario):
    exe = build_driver()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(scenario)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc {r.returncode}: {r.stdout}{r.stderr}"
    with open(outp, "rb") as f:
        return Out(f.read())


def header(w, h, slices, mips, flags, fmt):
    return struct.pack("<8I", int.from_bytes(b"LBC_", "big"), 0, w, h, slices, mips, 1 if flags & CUBEMAP else 0, fmt)


def mode_of(flags):
    return MO.STOCHASTIC if flags & STOCHASTIC else MO.SRGB if flags & SRGB else MO.LINEAR  # computeMip's order: stochastic wins whatever is_srgb says


def test_header_payload_order_modes_and_the_rgba8_case(tmp_path):
    rng = np.random.default_rng(6)
    G = COMPRESS | GENERATE_MIPMAPS
    cases = [  # w, h, slices, flags, scale_coverage_ref, the format
        (8, 8, 2, G | ALPHA | SRGB, 0.5, BC3),  # two slices; sRGB with coverage scaling
        (8, 4, 1, G | CUBEMAP, -0.5, BC1),  # six faces; linear
        (8, 8, 1, G | NORMALMAP | STOCHASTIC | SRGB, -0.5, BC5),  # stochastic wins over is_srgb
        (12, 4, 1, G | ALPHA | STOCHASTIC, 0.25, BC3),  # stochastic with coverage scaling; levels 6 x 2, 3 x 1 and 1 x 1 have texels outside
        (6, 4, 2, G | ALPHA | SRGB, 0.5, RGBA8),  # w not divisible by 4: the chains' pixels
        (8, 8, 1, GENERATE_MIPMAPS | SRGB, -0.5, RGBA8),  # options.compress off
    ]
    scenario, built = b"", []
    for w, h, slices, flags, ref_norm, _ in cases:
        blob, images = case(rng, w, h, slices, flags, ref_norm)
        scenario += blob
        built.append(images)
    out = run(tmp_path, scenario)
    for (w, h, slices, flags, ref_norm, fmt), images in zip(cases, built):
        what = f"{w} x {h}, {slices} slices, flags {flags}"
        assert out.u32() == fmt, what
        assert out.u32() == 0 and out.counted(np.uint8).tobytes() == LEAD, f"{what}: compress() refuses generate_mipmaps and leaves the stream alone"
        assert out.u32() == 1, what
        got = out.counted(np.uint8).tobytes()
        mips = MO.levels(w, h)
        assert got[:3] == LEAD and got[3:35] == header(w, h, slices, mips, flags, fmt), what
        chains = MO.chains(images, mode_of(flags), ref_norm)
        assert all(len(c) == mips for c in chains)
        if fmt == RGBA8:
            assert got[35:] == MO.flatten(chains).tobytes(), f"{what}: the chains' pixels, chain after chain in slice, face order"
            continue
        blocks = np.concatenate([TO.image_blocks(level) for chain in chains for level in chain])
        want = TO.encode(blocks, {BC1: TO.BC1, BC3: TO.BC3, BC5: TO.BC5}[fmt])[0]
        assert got[35:] == want.tobytes(), f"{what}: the blocks of every level of every chain in slice, face, mip order"
    assert out.done()


def test_refusals_leave_the_stream_alone(tmp_path):
    rng = np.random.default_rng(8)
    G = COMPRESS | GENERATE_MIPMAPS
    scenario = case(rng, 8, 8, 1, COMPRESS, want=False)[0]  # generate_mipmaps off: compress()'s case (it takes it: answered below)
    scenario += case(rng, 8, 8, 1, G, mips=2, want=False)[0]  # isValid: generated chains need src.mips == 1
    scenario += case(rng, 8, 8, 1, G | CUBEMAP | DROP_LAST_IMAGE, want=False)[0]  # isValid: an image is missing
    out = run(tmp_path, scenario)
    for k in range(3):
        assert out.u32() == BC1
        took = out.u32()
        before = out.counted(np.uint8).tobytes()
        assert took == (1 if k == 0 else 0) and (len(before) > 3 if k == 0 else before == LEAD)
        assert out.u32() == 0 and out.counted(np.uint8).tobytes() == before, "a refusal leaves the stream as it was"
    assert out.done()
