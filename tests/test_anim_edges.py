"""The animation sampler at its bit and clip-end edges, on the CPU: the clips of tests/anim_cases.py through three independent
statements of AnimationSampler::getRelativePose + the time advance, bit for bit -

  * the Python restatement of tests/test_animation.py (one rounding per operation, (float)(u64) rounded once, u32 time sums),
  * the port oracle (oracle/lmx_oracle.c),
  * the reference oracle: the reference's own sampler, sliced out of its tree at build time (oracle/ref/anim_shim.cpp) -

an independent decode of every field the builder packed, and a coverage tracker: the restatement notes which situations the case
list reaches, and every situation the cases were built for is asserted, so a case list that quietly loses an edge fails here.
The device runs the same cases in tests/test_gpu_anim_edges.py."""

import numpy as np
import pytest

from tests import anim_cases as AC
from tests import helpers as H
from tests.test_animation import f32, py_blend_stack, py_update_animable, u64_to_f32

CASES = AC.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def restated():
    """Every case through the Python restatement, once: {case name: {"update": [(pos, rot, times)], "stacks": (pos, rot)}} and the coverage set."""
    cov, out = set(), {}
    with np.errstate(all="ignore"):
        for c in CASES:
            res = {"update": [], "stacks": None}
            for (w, dt) in c.updates:
                rows = [py_update_animable(c.clips[k] if k >= 0 else None, t, dt, w, c.rel, cov) for (k, t) in c.animables()]
                res["update"].append((np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], np.uint32)))
            if c.run_stacks:
                rows = [py_blend_stack(c.clips, st, c.rel, cov) for st in c.stacks]
                res["stacks"] = (np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32))
            out[c.name] = res
    return out, cov


def all_clips():
    for c in CASES:
        for i, a in enumerate(c.clips):
            yield f"{c.name} clip {i}", a
    for i, a in enumerate(AC.end_clips("ff")):
        yield f"0xFF-tail clip {i}", a


def test_single_rounding_differs_from_double_rounding():
    """Why the restatement converts with u64_to_f32: through double, 2^55 + 2^31 + 1 first loses its last bit and then sits on a tie."""
    x = 2 ** 55 + 2 ** 31 + 1
    assert u64_to_f32(x) != f32(x) and float(u64_to_f32(x)) == 2.0 ** 55 + 2.0 ** 32 and float(f32(x)) == 2.0 ** 55


def test_every_field_decodes_to_what_the_builder_packed():
    """Independent of every sampler: the stream as one big integer, each field cut out by position."""
    n = 0
    for name, a in all_clips():
        for stream, frame_bits in (("translation", a["translations_frame_size_bits"]), ("rotation", a["rotations_frame_size_bits"])):
            raw = a[stream + "_stream"]
            big = int.from_bytes(bytes(raw), "little")
            data_bits = frame_bits * (a["frame_count"] + 1)
            for pos, nb, val in a["fields"][stream]:
                assert pos + nb <= data_bits and (big >> pos) & ((1 << nb) - 1) == val, f"{name} {stream} field at bit {pos}"
                n += 1
            assert len(raw) == (frame_bits * (a["frame_count"] + 2) + 7) // 8 + 8  # frame_count + 2 frames + 8 bytes
            tail = big >> data_bits
            if stream + "_stream_size" in a:
                assert tail == (1 << (8 * len(raw) - data_bits)) - 1 and a[stream + "_stream_size"] == (data_bits + 7) // 8
            else:
                assert tail == 0
        fc = a["frame_count"]
        assert len(a["root_pose_translations"]) == fc + 2 and len(a["root_pose_rotations"]) == fc + 2
        if "translation_stream_size" not in a:
            assert not a["root_pose_translations"][fc + 1].any() and not a["root_pose_rotations"][fc + 1].any()
    assert n > 5000


def test_gap_bits_complement_the_fields_next_to_them():
    a = AC.layout_clips()[0]
    for stream in ("translation", "rotation"):
        big = int.from_bytes(bytes(a[stream + "_stream"]), "little")
        fields = sorted(f for f in a["fields"][stream] if f[1])
        taken = set()
        for pos, nb, _ in fields:
            taken.update(range(pos, pos + nb))
        checked = 0
        for pos, nb, val in fields:
            if pos - 1 not in taken and pos > 0 and pos - 2 not in taken and pos >= 2:  # a gap of two or more: its upper half belongs to this field
                assert (big >> (pos - 1)) & 1 == 1 - (val & 1)
                checked += 1
            if pos + nb not in taken:
                assert (big >> (pos + nb)) & 1 == 1 - ((val >> (nb - 1)) & 1), f"{stream} bit above the field at {pos}"
                checked += 1
        assert checked > 100


def test_zero_tail_and_ff_tail_clips_agree_on_the_callers_frames():
    for z, f in zip(AC.end_clips("zero"), AC.end_clips("ff")):
        for stream, frame_bits in (("translation", z["translations_frame_size_bits"]), ("rotation", z["rotations_frame_size_bits"])):
            data_bits = frame_bits * (z["frame_count"] + 1)
            mask = (1 << data_bits) - 1
            assert int.from_bytes(bytes(z[stream + "_stream"]), "little") & mask == int.from_bytes(bytes(f[stream + "_stream"]), "little") & mask
            if frame_bits:
                assert data_bits % 8, "the last frame has to end inside a byte: that byte's tail is what the library must clear"
        n = z["frame_count"] + 1
        assert H.bits_equal(z["root_pose_rotations"][:n], f["root_pose_rotations"][:n]) and H.bits_equal(z["root_pose_translations"][:n], f["root_pose_translations"][:n])


def check_finite(*arrays):
    for x in arrays:
        assert np.isfinite(x).all(), "the cases are built to stay clear of NaN and infinity"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_port_oracle_matches_restatement(oracle_port, restated, case):
    want = restated[0][case.name]
    for (w, dt), (wp, wr, wt) in zip(case.updates, want["update"]):
        pos, rot, nt = AC.expected_update(oracle_port, case, w, dt)
        check_finite(pos, rot)
        for i in range(len(case.stacks)):
            assert H.bits_equal(pos[i], wp[i]) and H.bits_equal(rot[i], wr[i]), f"update weight {w} dt {dt} instance {i}: {case.stacks[i]}"
        assert np.array_equal(nt, wt), f"times after dt {dt}: {nt} != {wt}"
    if case.run_stacks:
        pos, rot = AC.expected_stacks(oracle_port, case)
        check_finite(pos, rot)
        for i in range(len(case.stacks)):
            assert H.bits_equal(pos[i], want["stacks"][0][i]) and H.bits_equal(rot[i], want["stacks"][1][i]), f"stack of instance {i}: {case.stacks[i]}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_sampler_matches_port_oracle(oracle_port, oracle_ref, case):
    """The reference's own getRelativePose (and its Time arithmetic in the advance) on the same clips. Where the case reads root-motion entry
    frame_count + 1 and oracle/_ref comes from a shim that does not pad it, the reference sampler's recorded poses stand in (AC.reference_values)."""
    oracle_ref = AC.reference_values(oracle_ref, case)
    for (w, dt) in case.updates:
        a, b = AC.expected_update(oracle_ref, case, w, dt), AC.expected_update(oracle_port, case, w, dt)
        assert H.bits_equal(a[0], b[0]) and H.bits_equal(a[1], b[1]), f"update weight {w} dt {dt}"
        assert np.array_equal(a[2], b[2]), f"times after dt {dt}: {a[2]} != {b[2]}"
    if case.run_stacks:
        a, b = AC.expected_stacks(oracle_ref, case), AC.expected_stacks(oracle_port, case)
        assert H.bits_equal(a[0], b[0]) and H.bits_equal(a[1], b[1])


def test_the_cases_reach_every_edge(restated):
    cov = restated[1]
    missing = []

    def need(*what):
        if what not in cov:
            missing.append(what)

    for stream in ("translation", "rotation"):
        for byte in range(8):
            for bit in range(8):
                need("pair", stream, byte, bit)
        for words in ("one word", "two words"):
            need("stitch", stream, words)
            need("ends on bit 63", stream, words)
        for w in AC.WIDTHS:
            need("width", stream, w)
    for ch in range(4):
        need("skipped_channel", ch)
    for sign in ("positive", "negative"):
        for rest in ("== 0", "< 0", "> 0"):
            need("rest", rest, sign)
    for d in ("d < 0", "d == 0", "d > 0"):
        need("frame pair", d)
    for kind in ("const translation", "translation", "const rotation", "rotation"):
        for use in (True, False):
            need("use_weight", kind, use)
    need("sample_idx == frame_count")
    need("f == 0")
    need("f != 0")
    need("skeleton mismatch")
    for where in ("inside", "frame_count + 0", "frame_count + 1"):
        need("root translation entry", where)
        need("root rotation entry", where)
    need("advance", "forward")
    need("advance", "backward")
    assert not missing, f"edges the case list no longer reaches: {missing}"


def test_rest_values_are_the_ones_the_rebuild_clip_was_built_for():
    """rest == 0 exactly, -2^-23 (one ulp of 1.0 below 0), -1 and a tiny positive one: from the track's fp32 arithmetic, not assumed."""
    y = f32(0.000345)
    one = f32(1)
    assert f32(one - f32(f32(one * one) + f32(y * y))) == f32(-2.0 ** -23)
    x = np.nextafter(one, f32(0))
    assert f32(one - f32(x * x)) == f32(2.0 ** -23)
    assert f32(one - f32(f32(x * x) + f32(y * y))) == 0


def test_clip_end_clips_clamp_onto_frame_count():
    """hi = frame_count - 0.00001f is frame_count itself from 257 frames on: what puts sample_idx on frame_count."""
    assert f32(f32(256) - f32(0.00001)) < 256
    for fc in (257, 300, 512):
        assert f32(f32(fc) - f32(0.00001)) == fc


def test_upper_clamp_is_the_same_from_a_double_expression():
    """For every frame_count lmx_anim_add admits (1 .. 2^24), (float)((double)frame_count - 0.00001) is (float)frame_count - 0.00001f: computing the
    clamp `hi` in double and rounding it changes nothing, so no case can tell the two apart (the mutant table) - and `hi` never
    exceeds frame_count. Above 2^24 neither holds (2^24 + 3: the fp32 expression gives 2^24 + 4), which is why lmx_anim_add stops there."""
    fc = np.arange(1, (1 << 24) + 1, dtype=np.uint32)
    single = fc.astype(np.float32) - np.float32(0.00001)
    double = (fc.astype(np.float64) - np.float64(np.float32(0.00001))).astype(np.float32)
    assert single.dtype == np.float32 and np.array_equal(single, double) and (single.astype(np.float64) <= fc).all()
    literal = (fc.astype(np.float64) - 0.00001).astype(np.float32)  # the double literal 0.00001 instead of the widened fp32 one
    assert np.array_equal(single, literal)
    odd = np.uint32((1 << 24) + 3)
    assert np.float32(odd) - np.float32(0.00001) == 2.0 ** 24 + 4 and np.float32(np.float64(odd) - 0.00001) == 2.0 ** 24 + 2


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("bones")], ids=lambda c: c.name)
def test_bone_tiling_expectations(oracle_port, case):
    """What the tiling cases are for, asserted on the oracle: the clip reaching the last bone writes it, the clip reaching bone n_bones leaves the
    pose the model's, and behind a shorter clip's max_bone the model's pose stays."""
    pos, rot = AC.expected_stacks(oracle_port, case)
    rel = AC.rel_array(case)
    n = case.n_bones
    assert not H.bits_equal(pos[0][n - 1], rel["pos"][n - 1]) or not H.bits_equal(rot[0][n - 1], rel["rot"][n - 1])  # instance 0: the last bone is written
    assert H.bits_equal(pos[1], rel["pos"]) and H.bits_equal(rot[1], rel["rot"])  # instance 1: no layer
    max_bone = max(int(x) for k in ("const_translations", "translations", "const_rotations", "rotations") for x in case.clips[1][k]["bone_index"])
    assert not H.bits_equal(rot[2][max_bone], rel["rot"][max_bone])
    if max_bone + 1 < n:
        assert H.bits_equal(pos[2][max_bone + 1 :], rel["pos"][max_bone + 1 :]) and H.bits_equal(rot[2][max_bone + 1 :], rel["rot"][max_bone + 1 :])
    if n < 196:
        assert H.bits_equal(pos[4], rel["pos"]) and H.bits_equal(rot[4], rel["rot"])  # instance 4: the clip reaches bone n_bones


def test_port_oracle_reproduces_committed_fixture(oracle_port):
    """tests/golden/anim_edges.npz: the reference sampler's poses of the layout and clip-end cases (tests/golden/make_golden_anim_edges.py)."""
    g = AC.Recorded()
    for c in CASES:
        if not c.golden:
            continue
        for (w, dt) in c.updates:
            got, want = AC.expected_update(oracle_port, c, w, dt), AC.expected_update(g, c, w, dt)
            assert H.bits_equal(got[0], want[0]) and H.bits_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), f"{c.name}: update weight {w}"
        for fn in (AC.expected_stacks, AC.expected_programs):
            got, want = fn(oracle_port, c), fn(g, c)
            assert H.bits_equal(got[0], want[0]) and H.bits_equal(got[1], want[1]), f"{c.name}: {fn.__name__}"
