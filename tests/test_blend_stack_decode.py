"""The blend stack decoder (lumixengine_amd/csrc/lmx_blend_stack.cpp, plain C++; lmx_anim_decode_blend_stack): hand-assembled streams in
the byte layout evalBlendStack reads (animation/controller.cpp:267-293) against the expected records, every rejection the header lists,
the layout of LmxBlendInstr, and a stand-alone sanitizer build that feeds the decoder truncated and bit-flipped streams. No GPU, and nothing
loaded into Python runs under a sanitizer: the fuzz driver is a program of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lumixengine_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build", "blend_stack")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DECODER = os.path.join(CSRC, "lmx_blend_stack.cpp")
END, SAMPLE, IK = 0, 1, 2  # anim::BlendStackInstructions, controller.h:58-62

SLOTS = [7, 0xFFFFFFFF, 3, 12]  # slot -> the library's animation id; slot 1 is empty
HASHES = [0x1111111111111111, 0xFEDCBA9876543210, 0x00000000DEADBEEF, 0x8000000000000001, 42]


def sample(slot, weight, time, looped):
    return struct.pack("<BIfIB", SAMPLE, slot, weight, time, looped)


def ik(alpha, target, leaf_hash, count):
    return struct.pack("<Bf3fQI", IK, alpha, *target, leaf_hash, count)


END_B = bytes([END])
VALID = [
    END_B,
    sample(0, 1.0, 12345, 1) + END_B,
    sample(2, 0.25, 0xFFFFFFF0, 0) + sample(3, 0.5, 0, 1) + END_B,
    ik(0.75, (1.0, -2.0, 3.5), HASHES[3], 3) + END_B,
    sample(0, 1.0, 100, 1) + ik(1.0, (0.0, 0.125, -0.5), HASHES[0], 32) + sample(3, 0.5, 7, 0) + ik(0.5, (9.0, 8.0, 7.0), 0x5555, 2) + END_B,
    sample(0, 1.0, 100, 2) + END_B + b"\x07garbage behind END",
]


@pytest.fixture(scope="module")
def api():
    from lumixengine_amd import api as a
    from lumixengine_amd import build

    if not os.path.exists(a.LIB_PATH):
        build.build()
    return a


def decode(api, stream, weight=1.0, capacity=64, slots=SLOTS, hashes=HASHES):
    return api.Skinning.decodeBlendStack(stream, slots, hashes, weight, capacity)


def test_round_trips(api):
    assert len(decode(api, VALID[0])) == 0
    r = decode(api, VALID[1])
    assert len(r) == 1 and (r[0]["op"], r[0]["animation"], r[0]["weight"], r[0]["time"], r[0]["looped"]) == (api.BLEND_SAMPLE_OP, 7, 1.0, 12345, 1)
    r = decode(api, VALID[2])
    assert [(int(x["animation"]), float(x["weight"]), int(x["time"]), int(x["looped"])) for x in r] == [(3, 0.25, 0xFFFFFFF0, 0), (12, 0.5, 0, 1)]
    r = decode(api, VALID[3], weight=0.3)
    assert len(r) == 1 and r[0]["op"] == api.BLEND_IK_OP and r[0]["leaf_bone"] == 3 and r[0]["bones_count"] == 3 and list(r[0]["target"]) == [1.0, -2.0, 3.5]
    assert r[0]["alpha"].view(np.uint32) == np.float32(np.float32(0.75) * np.float32(0.3)).view(np.uint32)  # alpha * RuntimeContext::weight in fp32, controller.cpp:280
    r = decode(api, VALID[4])
    assert [int(x["op"]) for x in r] == [1, 2, 1, 2]
    assert r[1]["leaf_bone"] == 0 and r[1]["bones_count"] == 32 and r[3]["leaf_bone"] == api.BONE_NONE and r[3]["bones_count"] == 2  # a hash that is not in the table
    assert r[2]["animation"] == 12 and r[2]["time"] == 7
    r = decode(api, VALID[5])
    assert len(r) == 1 and r[0]["looped"] == 1  # bool: any non-zero byte; bytes behind END are ignored
    assert not any(x["_pad"] for x in decode(api, VALID[4]))


@pytest.mark.parametrize("what, stream, code", [
    ("no END", sample(0, 1.0, 1, 1), 8),
    ("empty stream", b"", 8),
    ("unknown op", bytes([3]) + END_B, 8),
    ("unknown op behind a valid one", sample(0, 1.0, 1, 1) + bytes([0x80]) + END_B, 8),
    ("slot outside the table", sample(4, 1.0, 1, 1) + END_B, 8),
    ("empty slot", sample(1, 1.0, 1, 1) + END_B, 8),
    ("truncated SAMPLE", sample(0, 1.0, 1, 1)[:-1], 8),
    ("truncated IK", ik(1.0, (0, 0, 0), 42, 2)[:20] + END_B, 8),
    ("IK cut before its count", ik(1.0, (0, 0, 0), 42, 2)[:-4], 8),
])
def test_rejections(api, what, stream, code):
    with pytest.raises(api.LumixError) as e:
        decode(api, stream)
    assert e.value.code == code, what  # LMX_ERR_INVALID


def test_capacity(api):
    assert len(decode(api, VALID[4], capacity=4)) == 4
    with pytest.raises(api.LumixError) as e:
        decode(api, VALID[4], capacity=3)
    assert e.value.code == 5  # LMX_ERR_CAPACITY


def test_every_truncation_is_refused(api):
    for stream in VALID[:5]:
        for cut in range(len(stream)):
            with pytest.raises(api.LumixError):
                decode(api, stream[:cut])


def test_instruction_record_layout_matches_the_c_header(api, tmp_path):
    """LmxBlendInstr as the C compiler lays it out against api.BLEND_INSTR, and the constants next to it"""
    fields = ["op", "animation", "weight", "time", "looped", "alpha", "target", "leaf_bone", "bones_count", "_pad"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lumix_mi355.h"\nint main(void) {\nprintf("%zu", sizeof(LmxBlendInstr));\n'
                   + "".join(f'printf(" %zu", offsetof(LmxBlendInstr, {f}));\n' for f in fields)
                   + 'printf(" %u %u %u %d %u\\n", LMX_BLEND_SAMPLE, LMX_BLEND_IK, LMX_BONE_NONE, LMX_IK_MAX_BONES, LMX_ANIM_NONE);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[: 1 + len(fields)] == [api.BLEND_INSTR.itemsize] + [api.BLEND_INSTR.fields[f][1] for f in fields]
    assert got[0] == 48
    assert got[1 + len(fields):] == [api.BLEND_SAMPLE_OP, api.BLEND_IK_OP, api.BONE_NONE, api.IK_MAX_BONES, api.ANIM_NONE]
    assert (api.BLEND_SAMPLE_OP, api.BLEND_IK_OP) == (SAMPLE, IK)


def test_decoder_under_sanitizers_on_truncated_and_bit_flipped_streams(tmp_path):
    """The stand-alone driver (tests/cpp/blend_stack_fuzz.cpp), built with -fsanitize=address,undefined: every truncation and every
    single-bit flip of the valid streams is decoded or refused without a read outside the stream or a write outside the records."""
    if not os.path.exists(CLANG):
        pytest.skip("no host compiler for the decoder")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "blend_stack_fuzz")
    sources = [os.path.join(ROOT, "tests", "cpp", "blend_stack_fuzz.cpp"), DECODER]
    deps = sources + [os.path.join(CSRC, "lmx_blend_stack.h"), os.path.join(ROOT, "include", "lmx_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] + sources + ["-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(SLOTS)) + np.array(SLOTS, np.uint32).tobytes() + struct.pack("<I", len(HASHES)) + np.array(HASHES, np.uint64).tobytes())
        f.write(struct.pack("<I", len(VALID)))
        for s in VALID:
            f.write(struct.pack("<I", len(s)) + s)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "accepted" in r.stdout and " 0 accepted" not in r.stdout
