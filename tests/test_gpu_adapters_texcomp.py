"""GpuTextureCompressor (lumixengine_amd/host/gpu_texture_compressor.h) RUN: tests/cpp/run_texture_compressor.cpp fills Input-, Options- and
stream-shaped mocks (tests/cpp/lumix_compat_texcomp.h) from the cases written here and calls compress(), as the drivers of
tests/test_gpu_adapters_run.py do for the other adapters. Checked: the format choice of TextureCompressor::compress (:423-427), a size not
divisible by 4 staying RGBA8 with the images copied in the loop's order, the LBCHeader's bytes, and the payload of a 2-mip, 6-face batch in
slice, face, mip order against tests/texcomp_oracle.py; generate_mipmaps and an incomplete input are refused and leave the stream alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import texcomp_oracle as TO
from tests.adapters_run import BUILD, CPP, HOST, ROOT, Out, library, u32

pytestmark = pytest.mark.gpu
NORMALMAP, ALPHA, CUBEMAP, COMPRESS, GENERATE_MIPMAPS, DROP_LAST_IMAGE = 1, 2, 4, 8, 16, 32
RGBA8, BC1, BC3, BC5 = 4, 15, 17, 19  # gpu::TextureFormat
LEAD = bytes([1, 2, 3])  # what the driver's stream holds before compress appends


def build_driver():
    """tests/cpp/run_texture_compressor.cpp -> tests/_build/run_texture_compressor (the recipe of tests/adapters_run.build_exe)"""
    library()
    src, exe = os.path.join(CPP, "run_texture_compressor.cpp"), os.path.join(BUILD, "run_texture_compressor")
    os.makedirs(BUILD, exist_ok=True)
    deps = [src, os.path.join(HOST, "gpu_texture_compressor.h")] + [os.path.join(CPP, h) for h in ("adapter_run.h", "lumix_compat.h", "lumix_compat_texcomp.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("lumix_mi355.h", "lmx_types.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    lib_dir = os.path.join(ROOT, "lumixengine_amd")
    tmp = f"{exe}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-multichar", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + CPP, src, "-o", tmp, "-L" + lib_dir, "-llumix_mi355",
                    "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    os.replace(tmp, exe)
    return exe


def mip_size(v, mip):
    return max(v >> mip, 1)


def case(rng, w, h, slices, mips, flags, want=True):
    """-> (scenario bytes, images[(slice, face, mip)] uint8 (h, w, 4)); the scenario lists the images in mip, slice, face order"""
    faces = 6 if flags & CUBEMAP else 1
    images, blob = {}, u32(w, h, slices, mips, flags, int(want))
    for mip in range(mips):
        for s in range(slices):
            for f in range(faces):
                im = rng.integers(0, 256, (mip_size(h, mip), mip_size(w, mip), 4)).astype(np.uint8)
                images[(s, f, mip)] = im
                blob += im.tobytes()
    return blob, images


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


def in_loop_order(images, slices, faces, mips):
    return [images[(s, f, m)] for s in range(slices) for f in range(faces) for m in range(mips)]


def test_format_choice_header_and_payload_order(tmp_path):
    rng = np.random.default_rng(2)
    cases = [  # w, h, slices, mips, flags, the format compress chooses
        (8, 8, 1, 2, COMPRESS | ALPHA | CUBEMAP, BC3),  # a probe's shape: six faces, two mips (8 and 4)
        (8, 4, 1, 1, COMPRESS, BC1),
        (8, 4, 1, 1, COMPRESS | ALPHA, BC3),
        (8, 4, 2, 1, COMPRESS | NORMALMAP | ALPHA, BC5),  # is_normalmap comes first; two slices
        (6, 4, 1, 2, COMPRESS | ALPHA, RGBA8),  # w not divisible by 4
        (4, 10, 1, 1, COMPRESS | NORMALMAP, RGBA8),  # h not divisible by 4
        (8, 8, 1, 1, ALPHA, RGBA8),  # options.compress off
    ]
    scenario, built = b"", []
    for w, h, slices, mips, flags, _ in cases:
        blob, images = case(rng, w, h, slices, mips, flags)
        scenario += blob
        built.append(images)
    out = run(tmp_path, scenario)
    for (w, h, slices, mips, flags, fmt), images in zip(cases, built):
        what = f"{w} x {h}, flags {flags}"
        assert out.u32() == fmt, what
        assert out.u32() == 1, what
        got = out.counted(np.uint8).tobytes()
        assert got[:3] == LEAD and got[3:35] == header(w, h, slices, mips, flags, fmt), what
        ordered = in_loop_order(images, slices, 6 if flags & CUBEMAP else 1, mips)
        if fmt == RGBA8:
            assert got[35:] == b"".join(im.tobytes() for im in ordered), f"{what}: the images as they are, in slice, face, mip order"
            continue
        blocks = np.concatenate([TO.image_blocks(im) for im in ordered])
        want = TO.encode(blocks, {BC1: TO.BC1, BC3: TO.BC3, BC5: TO.BC5}[fmt])[0]
        assert got[35:] == want.tobytes(), f"{what}: the blocks of every image in slice, face, mip order"
    assert out.done()


def test_refusals_leave_the_stream_alone(tmp_path):
    rng = np.random.default_rng(4)
    scenario = case(rng, 8, 8, 1, 1, COMPRESS | GENERATE_MIPMAPS, want=False)[0]  # mip generation stays with the engine
    scenario += case(rng, 8, 8, 1, 2, COMPRESS | CUBEMAP | DROP_LAST_IMAGE, want=False)[0]  # isValid: an image is missing
    out = run(tmp_path, scenario)
    for fmt in (BC1, BC1):
        assert out.u32() == fmt and out.u32() == 0
        assert out.counted(np.uint8).tobytes() == LEAD
    assert out.done()
