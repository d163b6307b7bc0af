"""The particle program decoder (lumixengine_amd/csrc/lmx_particle_program.cpp, plain C++): every rejection include/lumix_mi355.h lists
for lmx_particles_set_program, and a stand-alone sanitizer build that feeds it truncated and bit-flipped streams. No GPU, and nothing
loaded into Python runs under a sanitizer: the fuzz driver is a program of its own."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import particle_asm as A
from tests.particle_asm import CH, REG, LIT, SYS, GLOB, OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lumixengine_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build", "particle_program")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DECODER = os.path.join(CSRC, "lmx_particle_program.cpp")


def compiler():
    if os.path.exists(CLANG):
        return CLANG
    pytest.skip("no host compiler for the decoder")


def build(target, sources, extra):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, target)
    deps = sources + [os.path.join(CSRC, "lmx_particle_program.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        r = subprocess.run([compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-I" + CSRC] + extra + sources + ["-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(build("libparticle_shim.so", [os.path.join(ROOT, "tests", "cpp", "particle_program_shim.cpp"), DECODER], ["-fPIC", "-shared"]))
    lib.particle_shim_decode.restype = C.c_int
    lib.particle_shim_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p]
    return lib


def header(p, size=None, n_emitters=2, n_globals=2, **over):
    h = dict(size=len(p.bytes) if size is None else size, emit_offset=p.emit_offset, output_offset=p.output_offset, channels=p.channels, registers=p.registers,
             outputs=p.outputs, emit_inputs=p.emit_inputs, n_emitters=n_emitters, n_globals=n_globals)
    h.update(over)
    return np.array(list(h.values()), np.uint32)


def decode(shim, p, **over):
    buf = np.frombuffer(p.bytes, np.uint8).copy()
    err = C.create_string_buffer(256)
    n = C.c_uint32()
    rc = shim.particle_shim_decode(buf.ctypes.data, header(p, **over).ctypes.data, err, 256, C.byref(n))
    return rc, err.value.decode(), n.value


def prog(update=(), emit=(), output=(), **kw):
    kw.setdefault("channels", 4)
    kw.setdefault("registers", 4)
    kw.setdefault("outputs", 2)
    return A.Program(update, emit, output, **kw)


COND = A.gt(REG(0), CH(0), LIT(0.0))
VALID = [
    prog([A.add(CH(0), CH(0), SYS(A.TIME_DELTA)), COND, A.cmp(REG(0), [A.mul(CH(1), CH(1), GLOB(1)), A.cmp_else(CH(1), [A.KILL], [A.not_(REG(1), CH(2)), A.cmp(REG(1), [A.KILL])])])],
         [A.mov(CH(0), SYS(A.EMIT_INDEX)), A.rand(CH(1), 0.0, 1.0), A.cmp(CH(0), [A.mov(CH(2), LIT(1.0))])],
         [A.mov(OUT(0), CH(0)), A.gradient(OUT(1), CH(1), [0.0, 0.5, 1.0], [1.0, 2.0, 0.0]), COND, A.cmp_else(REG(0), [A.mov(OUT(1), OUT(0))], [A.sin(OUT(0), CH(3))])]),
    prog([A.madd(CH(0), CH(1), LIT(2.0), REG(0)), A.mix(REG(1), CH(0), GLOB(0), SYS(A.TOTAL_TIME)), A.blend(CH(2), CH(0), CH(1), REG(1)), A.rand(REG(2), -1.0, 1.0),
          A.gradient(REG(3), REG(2), [0.0, 1.0], [0.0, 1.0]), A.noise(CH(3), REG(3)), A.mod(CH(3), CH(3), CH(0))], [], [A.rand(OUT(0), 0.0, 1.0), A.sqrt(OUT(1), CH(3))]),
]


def test_valid_programs_decode(shim):
    for p in VALID:
        rc, err, n = decode(shim, p)
        assert rc == 0 and n > 3, err


REJECTED = {
    "stream type out of range": prog([A.add(CH(0), A.stream(9, 0), CH(1))]),
    "stream type NONE": prog([A.add(CH(0), A.stream(A.NONE, 0), CH(1))]),
    "output read by a whole-chunk instruction": prog(output=[A.add(OUT(0), OUT(1), CH(1))]),
    "literal where getStream is used": prog([A.sin(CH(0), LIT(1.0))]),
    "system value into an output by MOV": prog(output=[A.mov(OUT(0), SYS(A.TIME_DELTA))]),
    "global into a channel by MOV": prog([A.mov(CH(0), GLOB(0))]),
    "condition that is a literal": prog([A.cmp(LIT(1.0), [A.KILL])]),
    "channel index >= 16": prog([A.add(CH(16), CH(0), CH(1))], channels=16),
    "channel index past the emitter's": prog([A.add(CH(4), CH(0), CH(1))]),
    "register index >= 16": prog([A.add(REG(16), CH(0), CH(1))], registers=16),
    "register index past the emitter's": prog([A.add(REG(4), CH(0), CH(1))]),
    "output index >= outputs_count": prog(output=[A.mov(OUT(2), CH(0))]),
    "output in the update program": prog([A.mov(OUT(0), CH(0))]),
    "output in the emit program": prog(emit=[A.mov(OUT(0), CH(0))]),
    "system value index": prog([A.add(CH(0), SYS(7), CH(1))]),
    "global index": prog([A.add(CH(0), GLOB(2), CH(1))]),
    "block size past the program": prog([COND, bytes([A.OP["CMP"]]) + REG(0) + struct.pack("<H", 4000) + A.KILL + A.END]),
    "false block size past the program": prog([COND, bytes([A.OP["CMP_ELSE"]]) + REG(0) + struct.pack("<HH", 2, 4000) + A.KILL + A.END + A.END]),
    "block without END at its end": prog([COND, bytes([A.OP["CMP"]]) + REG(0) + struct.pack("<H", 1) + A.KILL]),
    "nesting deeper than the stack": prog([COND, A.cmp(REG(0), [A.cmp(CH(0), [A.cmp(CH(0), [A.cmp(CH(0), [A.cmp(CH(0), [A.KILL])])])])])]),
    "conditional in the true arm of a CMP_ELSE": prog([COND, A.cmp(REG(0), [A.cmp_else(CH(0), [A.cmp(CH(1), [A.KILL])], [])])]),
    "GRADIENT with 9 keys": prog(output=[A.gradient(OUT(0), CH(0), [float(i) for i in range(9)], [0.0] * 9)]),
    "GRADIENT with 1 key": prog(output=[A.gradient(OUT(0), CH(0), [0.0], [0.0])]),
    "GRADIENT into a channel": prog([A.gradient(CH(0), CH(1), [0.0, 1.0], [0.0, 1.0])]),
    "GRADIENT inside a block": prog([COND, A.cmp(REG(0), [A.gradient(REG(1), CH(1), [0.0, 1.0], [0.0, 1.0])])]),
    "BLEND inside a block": prog([COND, A.cmp(REG(0), [A.blend(CH(0), CH(0), CH(1), CH(2))])]),
    "EMIT target out of range": prog([COND, A.cmp(REG(0), [A.emit(2, [A.mov(OUT(0), CH(0))])])]),
    "emit-output block larger than 16 values": prog([COND, A.cmp(REG(0), [A.emit(1, [A.mov(OUT(16), CH(0))])])]),
    "KILL outside a conditional block": prog([A.KILL]),
    "EMIT outside a conditional block": prog([A.emit(1, [])]),
    "NOT outside a conditional block": prog([A.not_(REG(0), CH(0))]),
    "KILL in the emit program": prog(emit=[A.KILL]),
    "KILL in the output program": prog(output=[COND, A.cmp(REG(0), [A.KILL])]),
    "destination LITERAL": prog([A.add(LIT(0.0), CH(0), CH(1))]),
    "destination GLOBAL": prog([A.add(GLOB(0), CH(0), CH(1))]),
    "destination SYSTEM_VALUE": prog([COND, A.cmp(REG(0), [A.mov(SYS(0), CH(1))])]),
    "instruction type out of range": prog([bytes([29]) + CH(0) + CH(1)]),
}


@pytest.mark.parametrize("what", sorted(REJECTED))
def test_rejections(shim, what):
    rc, err, _ = decode(shim, REJECTED[what])
    assert rc == 1 and err.startswith("particle program"), (what, rc, err)


def test_program_without_its_end(shim):
    p = VALID[1]
    for size in (len(p.bytes) - 1, p.output_offset, p.emit_offset + 0, 1, 0):  # the output, emit or update program loses its END
        rc, err, _ = decode(shim, p, size=size)
        assert rc == 1, (size, err)
    assert decode(shim, p, emit_offset=len(p.bytes))[0] == 1 and decode(shim, p, output_offset=len(p.bytes) + 5)[0] == 1
    assert decode(shim, p, channels=17)[0] == 1 and decode(shim, p, registers=17)[0] == 1 and decode(shim, p, registers=10, emit_inputs=7)[0] == 1


def test_mesh_and_spline_are_flagged_for_refusal(shim):
    assert decode(shim, prog([COND, A.cmp(REG(0), [A.mesh(CH(0), REG(0), 1)])]))[0] == 2
    assert decode(shim, prog(output=[A.spline(OUT(0), CH(0), 2)]))[0] == 2
    assert decode(shim, prog([COND, A.cmp(REG(0), [A.emit(1, [A.mov(OUT(3), CH(0))]), A.KILL])]))[0] == 3  # (accepted: the shim only tells it apart)
    assert decode(shim, prog([COND, A.cmp(REG(0), [A.emit(1, [])] * 9)]))[0] == 1  # more than 8 EMIT instructions


def test_decoder_under_sanitizers_on_truncated_and_bit_flipped_streams(tmp_path):
    """The stand-alone driver (tests/cpp/particle_program_fuzz.cpp), built with -fsanitize=address,undefined: every truncation and every
    single-bit flip of the valid programs is accepted or refused without a read outside the stream."""
    exe = build("particle_program_fuzz", [os.path.join(ROOT, "tests", "cpp", "particle_program_fuzz.cpp"), DECODER], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                                                                    "-fno-omit-frame-pointer"])
    path = tmp_path / "programs.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(VALID)))
        for p in VALID:
            f.write(header(p).tobytes())
            f.write(p.bytes)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "accepted" in r.stdout
