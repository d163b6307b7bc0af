"""createCommands (renderer/pipeline.cpp:2747-3320) without a GPU: the numpy oracle (tests/draw_oracle.py) on the hand-made pair
sequences of tests/draw_cases.py - run boundaries derived by hand from the reference's while loops - plus the layout of the records it
writes, and the ISA of draw_kernels.hip (bit-exact: no fused multiply-add). The built sequences of draw_cases.SEAM_SEQUENCES - a chosen
scan state placed on the first pair behind a wave, tile or scan-round edge of the device's scan - are held the same way: the walk must
cut the runs the builder predicts, and a tracker of the state confirms that every edge class meets every situation."""
import numpy as np
import pytest

from tests import draw_cases as DC
from tests import draw_oracle as DO
from tests.test_isa_no_fma import FMA, isa_of, kernels


def run_case(name):
    keys, values, n_batches, want = DC.arrays(name)
    sc, dt, lod, tr = DC.tables()
    T = DO.Tables(sc, dt, lod, tr)
    runs, data, groups = DO.create_commands(keys, values, DC.view(), n_batches, T)
    return keys, values, want, runs, data, (sc, dt, lod, tr)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_run_boundaries(name):
    keys, values, want, runs, data, _ = run_case(name)
    got = [(int(r["first_pair"]), int(r["pair_count"]), int(r["kind"])) for r in runs]
    assert got == want
    # slices: back to back in run order, 16-byte aligned, stride of the kind; AUTOINSTANCED runs own no bytes of the instance buffer
    at = 0
    for r in runs:
        if r["kind"] == DC.AUTO:
            assert r["stride"] == 48
            continue
        assert r["data_offset"] == at and at % 16 == 0 and r["stride"] == DO.STRIDE.get(int(r["kind"]), 0)
        at += (int(r["pair_count"]) * int(r["stride"]) + 15) & ~15
    assert len(data) == at
    n = len(keys)
    step = max((n + DC.CASES[name][1] - 1) // DC.CASES[name][1], 1)
    for r in runs:  # no run crosses a slice of the pairs
        assert int(r["first_pair"]) // step == (int(r["first_pair"]) + int(r["pair_count"]) - 1) // step == int(r["batch"])


def test_static_run_writes_the_heads_material_and_each_pairs_transform():
    keys, values, want, runs, data, (sc, dt, lod, tr) = run_case("MESH head swallows SKINNED pairs of its masked key")
    rec = data.view(np.uint32).reshape(3, 12)
    head_material = dt["material_index"][sc["material_offset"][1] + 0]
    assert np.all(rec[:, 11] == head_material)
    cam = np.array([3.0, -2.0, 7.5])
    for k, e in enumerate((1, 2, 3)):
        assert np.array_equal(rec[k, 0:4], tr["rot"][e].view(np.uint32))
        assert np.array_equal(rec[k, 4:7], (tr["pos"][e] - cam).astype(np.float32).view(np.uint32))
        assert rec[k, 7] == np.float32(lod[e] - dt["mesh_lod"][0]).view(np.uint32)  # the HEAD's mesh index (0), each entity's lod


def test_moved_and_skinned_records():
    keys, values, want, runs, data, (sc, dt, lod, tr) = run_case("moved MESH heads end at full-key breaks")
    rec = data[: 2 * 96].view(np.uint32).reshape(2, 24)
    assert np.all(rec[:, 11] == 0)
    for k, e in enumerate((16, 1)):
        assert rec[k, 23] == dt["material_index"][sc["material_offset"][e]]  # each entity's own
        assert np.array_equal(rec[k, 12:16], dt["prev"]["rot"][e].view(np.uint32)) and rec[k, 19] == rec[k, 7]
    keys, values, want, runs, data, (sc, dt, lod, tr) = run_case("SKINNED head swallows a MESH pair of its key")
    assert runs[0]["stride"] == 92 and runs[1]["data_offset"] == 192  # 2 x 92 = 184 -> 192
    rec = data[:184].view(np.uint32).reshape(2, 23)
    for k, e in enumerate((1, 2)):
        assert rec[k, 0] == dt["material_index"][sc["material_offset"][e] + 1] and rec[k, 1] == dt["bones_handle"][e] and rec[k, 2] == dt["bones_offset"][e]
    assert not data[184:192].any()


def test_decal_runs_are_two_ended():
    keys, values, want, runs, data, (sc, dt, lod, tr) = run_case("decal run, mixed")
    assert [int(r["front_count"]) for r in runs] == [3, 1]
    cam = np.array([3.0, -2.0, 7.5])
    rec = data[: 6 * 52].view(np.uint32).reshape(6, 13)
    order = [0, 1, 2, 8, 12, 11]  # front in walk order, then the back part: filled downwards from the end
    for k, e in enumerate(order):
        assert np.array_equal(rec[k, 0:3], (tr["pos"][e] - cam).astype(np.float32).view(np.uint32)), k
    assert np.all(rec[:, 12] == dt["decal_material"][0])  # the head's material
    off = int(runs[1]["data_offset"])
    assert off == 320  # 312 -> 320
    rec = data[off : off + 4 * 68].view(np.uint32).reshape(4, 17)
    for k, e in enumerate([3, 11, 15, 12]):
        assert np.array_equal(rec[k, 0:3], (tr["pos"][e] - cam).astype(np.float32).view(np.uint32)), k
        assert np.array_equal(rec[k, 12:16], dt["curve_bezier"][e].view(np.uint32))
    keys, values, want, runs, data, _ = run_case("decal run, all front")
    assert runs[0]["front_count"] == 4
    keys, values, want, runs, data, _ = run_case("decal run, all back")
    assert runs[0]["front_count"] == 0


def test_near_plane_is_left_to_right_fp32():
    from lumixengine_amd import api

    fr = np.zeros(1, api.SHIFTED_FRUSTUM)
    fr["xs"][0, 0], fr["ys"][0, 0], fr["zs"][0, 0], fr["ds"][0, 0] = 0.3, -0.7, 0.64, 1.0e-3
    fr["origin"][0] = (1.0e6, 2.0, -3.0)
    rng = np.random.default_rng(2)
    pos = rng.uniform(-40, 40, size=(500, 3)) + fr["origin"][0]
    got = DO.intersect_near_plane(fr, pos, np.full(500, 5.0, np.float32))
    f32 = np.float32
    for i in range(500):
        x, y, z = (f32(pos[i, k] - fr["origin"][0, k]) for k in range(3))
        d = f32(f32(f32(f32(f32(0.3) * x) + f32(f32(-0.7) * y)) + f32(z * f32(0.64))) + f32(1.0e-3))
        assert got[i] == (abs(d) < f32(5.0))


def test_group_fill():
    sc, dt, lod, tr = DC.tables()
    offsets = np.array([0, 0, 3, 3, 5], np.uint32)
    gv = np.array([DC.val(4, 0, 1), DC.val(5, 0, 0), DC.val(6, 0, 1), DC.val(7, 0, 0), DC.val(1, 0, 0)], np.uint64) & np.uint64(~(31 << 32) & (2**64 - 1))
    T = DO.Tables(sc, dt, lod, tr, offsets, gv)
    keys = np.array([DC.key(0, 1 | (1 << 55)), DC.key(0, 3 | (1 << 55))], np.uint64)
    values = np.array([DC.val(1, DC.AUTO), DC.val(3, DC.AUTO)], np.uint64)
    runs, data, groups = DO.create_commands(keys, values, DC.view(), 1, T)
    assert len(data) == 0 and len(groups) == 5 * 48
    assert [(int(r["group"]), int(r["total_count"]), int(r["data_offset"]), int(r["head_entity"]), int(r["mesh_idx"])) for r in runs] == [(1, 3, 0, 4, 1), (3, 2, 144, 7, 0)]
    rec = groups.view(np.uint32).reshape(5, 12)
    for j, (e, first_mesh) in enumerate([(4, 1), (5, 1), (6, 1), (7, 0), (1, 0)]):  # Mesh::lod and the mesh index come from the group's FIRST renderable
        assert rec[j, 7] == np.float32(lod[e] - dt["mesh_lod"][first_mesh]).view(np.uint32)
        assert rec[j, 11] == dt["material_index"][sc["material_offset"][e] + first_mesh]


@pytest.mark.parametrize("name", list(DC.SEAM_SEQUENCES))
def test_seam_sequences_cut_where_the_builder_predicts(name):
    keys, values, windows, filler = DC.SEAM_SEQUENCES[name]()
    sc, dt, lod, tr = DC.tables()
    go, gv = DC.instancer()
    T = DO.Tables(sc, dt, lod, tr, go, gv)
    for n_batches in (1, 8):
        DC.check_windows(name, DO.walk(keys, values, n_batches, [0, 0, 1, 1], T), windows, filler, len(keys), n_batches)
    runs, data, groups = DO.create_commands(keys, values, DC.view(), 1, T)
    DC.check_windows(name, runs, windows, filler, len(keys))
    big = [f for f in filler if f[2] in (DC.DECAL, DC.CURVE)]
    assert sorted(f[2] for f in big) == [DC.DECAL, DC.CURVE] and all(f[1] >= 3 * 256 + 255 for f in big)  # three whole tiles inside each
    for first, count, kind, front in big:
        r = runs[runs["first_pair"] == first][0]
        assert (int(r["pair_count"]), int(r["front_count"])) == (count, front) and 0 < front < count
    assert {DC.MESH, DC.MOVED} <= {f[2] for f in filler} and any(f[2] == DC.MOVED and f[1] % 2 for f in filler)


def test_seam_sequences_cover_every_situation_at_every_seam_class():
    """scan_trace follows {streak, blocked} pair by pair; it only counts what the sequences reach, the expected runs never come from it."""
    seen = {"wave": set(), "tile": set(), "round": set(), "carry": set(), 63: set(), 1: set(), 255: set(), 257: set()}
    buckets = {}
    for name, build in DC.SEAM_SEQUENCES.items():
        keys, values, windows, _ = build()
        trace = DC.scan_trace(keys, values)
        for b, s, c, k, *_ in windows:
            assert trace[b] == (s, c, k), f"{name}: pair {b} meets {trace[b]}, not {DC.situation_name(s, c, k)}"
            buckets.setdefault((s, c, k), set()).add(int(keys[b]) >> 56 >= DC.DEPTH)
        if name.startswith("round carry"):  # the state set up in front of the round seam reaches pair 65 792 through a whole tile that leaves it alone
            b, s = windows[0][:2]
            assert b == DC.CARRY_AT and all(t[0] == s for t in trace[DC.ROUND - 1:b + 1]), name
            seen["carry"].add(trace[b])
        for b in range(1, len(keys)):
            cls = DC.seam_class(b)
            if cls:
                seen[cls].add(trace[b])
        for lane, mod in ((63, 64), (1, 64), (255, 256), (257, 256)):  # the shifted copies: the last lane in front of a seam, the second behind it
            seen[lane] |= {trace[b] for b, *_ in windows if b % mod == lane % mod and (mod == 256 or (b - lane) % 256)}
    want = set(DC.SITUATIONS)
    assert len(want) == 36
    for cls in ("wave", "tile", 63, 1, 255, 257):
        assert seen[cls] >= want, f"{cls}: missing {[DC.situation_name(*x) for x in sorted(want - seen[cls])]}"
    assert len(DC.ROUND_SITUATIONS) == 12 and {(s, c) for s, c, k in DC.ROUND_SITUATIONS} == {(s, c) for s in range(4) for c in range(3)}
    assert {k for s, c, k in DC.ROUND_SITUATIONS} == {DC.ONE, DC.UNMOVED, DC.OTHER}
    for cls in ("round", "carry"):
        assert seen[cls] >= set(DC.ROUND_SITUATIONS), f"{cls}: missing {[DC.situation_name(*x) for x in sorted(set(DC.ROUND_SITUATIONS) - seen[cls])]}"
    # every situation meets a plain and a depth-sorted bucket (the masked key is another there)
    assert all(buckets[x] == {False, True} for x in want), [DC.situation_name(*x) for x in want if buckets[x] != {False, True}]


def test_draw_kernels_contain_no_fused_multiply_add(tmp_path):
    ks = kernels(isa_of("draw_kernels.hip", tmp_path))
    names = [n for n in ks if "k_draw_" in n]
    assert len(names) >= 7, list(ks)
    for n in names:
        bad = [l for l in ks[n] if FMA.search(l)]
        assert not bad, f"{n}: {bad[:5]}"
