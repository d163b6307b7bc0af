"""GpuAnimationCompressor (lumixengine_amd/host/gpu_animation_compressor.h) RUN: tests/cpp/run_animation_compressor.cpp fills the
Array<Array<Key>>- and stream-shaped mocks of tests/cpp/lumix_compat_animcomp.h from the scenario written here - the keys per bone, per
sample, as the importer holds them, an empty array for a bone without keys - and calls compress() and write(). Checked: each clip's .ani
bytes against tests/animcomp_oracle.py's (header magic and version, the skeleton path, fps, samples - 1, flags, the interleaved records,
both streams), for a batch of clips of different lengths over one skeleton; a refused clip between them returning false with its status
and leaving the stream alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import animcomp_cases as AC
from tests import animcomp_oracle as AO
from tests.adapters_run import BUILD, CPP, HOST, ROOT, Out, library, u32

pytestmark = pytest.mark.gpu
LEAD = bytes([1, 2, 3])  # what the driver's stream holds before the adapter appends
PATH = "models/walker.fbx"


def build_driver():
    """tests/cpp/run_animation_compressor.cpp -> tests/_build/run_animation_compressor (the recipe of tests/adapters_run.build_exe)"""
    library()
    src, exe = os.path.join(CPP, "run_animation_compressor.cpp"), os.path.join(BUILD, "run_animation_compressor")
    os.makedirs(BUILD, exist_ok=True)
    deps = [src, os.path.join(HOST, "gpu_animation_compressor.h")] + [os.path.join(CPP, h) for h in ("adapter_run.h", "lumix_compat.h", "lumix_compat_animcomp.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("lumix_mi355.h", "lmx_types.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    lib_dir = os.path.join(ROOT, "lumixengine_amd")
    tmp = f"{exe}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-multichar", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + CPP, src, "-o", tmp, "-L" + lib_dir, "-llumix_mi355",
                    "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    os.replace(tmp, exe)
    return exe


def test_ani_bytes_of_a_batch_over_one_skeleton(tmp_path):
    nb = 19
    rng = np.random.default_rng(3)
    hashes = rng.integers(1, 2 ** 63, nb).astype(np.uint64)
    no_keys = (0, 7, 18)
    base = AC.mixed("adapter", 70, nb, 51, no_keys=no_keys, unit=False)
    bind, has = base["bind"], base["has_keys"]
    floats = AC.as_floats(base["keys"])
    wide = floats[:40].copy()
    wide[5, 3, 1] = 3.0e5  # a quotient of 2^32: refused
    clips = [(floats, 30.0, 0, 1.0, 1.0), (wide, 24.0, 5, 1.0, 1.0), (floats[:33], 60.0, 7, 0.5, 2.0), (floats[:1], 30.0, 0, 1.0, 1.0)]
    scenario = u32(nb, len(clips)) + bind.tobytes() + hashes.tobytes() + u32(len(PATH)) + PATH.encode()
    for k, fps, flags, te, re in clips:
        scenario += u32(len(k)) + struct.pack("<fIff", fps, flags, te, re)
        for b in range(nb):
            scenario += u32(int(has[b])) + (np.ascontiguousarray(k[:, b]).tobytes() if has[b] else b"")
    exe = build_driver()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(scenario)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc {r.returncode}: {r.stdout}{r.stderr}"
    with open(outp, "rb") as f:
        out = Out(f.read())
    assert out.u32() == 1, "the batch ran"
    for i, (k, fps, flags, te, re) in enumerate(clips):
        want = AO.compress(k, bind, has, te, re)
        ok, status, got = out.u32(), out.u32(), out.counted(np.uint8).tobytes()
        assert status == want["status"], i
        if want["status"]:
            assert i == 1 and status == AO.QUOTIENT_RANGE and ok == 0 and got == LEAD, "a refused clip leaves the stream as it was"
            continue
        file = AO.ani_file(want, hashes, PATH, fps, flags)
        assert ok == 1 and got[:3] == LEAD
        assert got[3:11] == struct.pack("<II", 0x5F4C4146, 8) and got[11:11 + len(PATH) + 1] == PATH.encode() + b"\0"
        assert got[3:] == file, f"clip {i}: {len(got) - 3} vs {len(file)} bytes, first difference at {next((j for j, (a, b) in enumerate(zip(got[3:], file)) if a != b), None)}"
        assert want["n_const_translations"] and want["n_const_rotations"] and (len(k) == 1 or (want["n_translations"] and want["n_rotations"])), "both kinds of record are interleaved"
    assert out.done()
