"""The seams of the draw encoder's scan (draw_kernels.hip): the state {streak, blocked} composed by wave shuffles (every 64 pairs), through
LDS across the waves of a tile (every 256), by k_draw_tile_scan across tiles in rounds with a carry (every 65 536), and restarted at batch
starts. tests/draw_cases.py places each of the 36 situations (carried state x key class x kind of the pair) on the first pair behind such a
seam, on the lane in front of it and on the second lane behind it; the run list around the pair is the one the builder derives from the
reference's walk (a failure names the seam and the situation), and run records, instance buffer and group buffer equal the numpy oracle's
byte for byte - which tests/test_draw_oracle_vs_ref.py pins to the reference on these very sequences. Also: batch starts on and next to a
seam, runs that own whole tiles, and the instancer CSR with group edges around a tile edge of k_draw_groups."""
import numpy as np
import pytest

from tests import draw_cases as DC
from tests import draw_oracle as DO
from tests.test_gpu_draw_commands import assert_equal_bytes, upload_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    sc, dt, lod, tr = DC.tables()
    sk, dc = upload_tables(gpu_ctx, sc, dt, tr, DC.N_ENTITIES)
    return dc, (sc, dt, lod, tr)


def encode(scene, name, keys, values, n_batches, go=None, gv=None):
    """runPairs twice (identical bytes), everything against the oracle; -> (the device's run records, instance buffer, the oracle's runs)"""
    dc, (sc, dt, lod, tr) = scene
    dc.runPairs(DC.view(), keys, values, n_batches, go, gv)
    runs, data, groups = dc.readRuns(), dc.readInstanceData(), dc.readGroupData()
    dc.runPairs(DC.view(), keys, values, n_batches, go, gv)
    again = (dc.readRuns().tobytes(), dc.readInstanceData().tobytes(), dc.readGroupData().tobytes())
    assert again == (runs.tobytes(), data.tobytes(), groups.tobytes()), f"{name}: two runs in a row differ"
    return runs, data, DO.create_commands(keys, values, DC.view(), n_batches, DO.Tables(sc, dt, lod, tr, go, gv))


def check_tiling(name, runs, n):
    """the runs tile [0, n): the first wrong head flag shows as the first gap or overlap"""
    first, count = runs["first_pair"].astype(np.int64), runs["pair_count"].astype(np.int64)
    ends = np.concatenate([[0], first + count])
    bad = np.flatnonzero(ends[:-1] != first)
    assert not len(bad), f"{name}: run {bad[0]} starts at pair {first[bad[0]]}, the run before it ends at {ends[bad[0]]}"
    assert ends[-1] == n, f"{name}: the last run ends at pair {ends[-1]} of {n}"


SEAM_RUNS = [(name, nb) for name in DC.SEAM_SEQUENCES for nb in ((1,) if name.startswith("round") else (1, 8))]


@pytest.mark.parametrize("name,n_batches", SEAM_RUNS, ids=[f"{name}, {nb} batches" for name, nb in SEAM_RUNS])
def test_state_carried_across_a_seam(scene, name, n_batches):
    keys, values, windows, filler = DC.SEAM_SEQUENCES[name]()
    go, gv = DC.instancer()
    runs, data, want = encode(scene, name, keys, values, n_batches, go, gv)
    DC.check_windows(name, runs, windows, filler, len(keys), n_batches)  # names the seam and the situation
    check_tiling(name, runs, len(keys))
    assert_equal_bytes(scene[0], want, name)


STRETCHES = ("equal-key unmoved MESH", "blocked segment", "equal-key one-pair heads")


@pytest.mark.parametrize("stretch", STRETCHES)
@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("b", [192, 512], ids=["wave seam", "tile seam"])
def test_batch_start_on_a_seam(scene, b, d, stretch):
    """Three batches of b + d pairs: the second starts on the last lane in front of the seam, on the seam, on the lane behind it, while a
    stretch of 16 pairs lies across [b - 8, b + 8). The reference restarts its walk there (pipeline.cpp:2810)."""
    step = b + d
    n = 3 * step - 1
    q = DC.Seq()
    q.run(b - 8, DC.MESH, range(16), bucket=DC.PLAIN if d else DC.DEPTH)
    if stretch == STRETCHES[0]:
        q.run(16, DC.MESH, range(3, 16), 1)
        want = [(b - 8, step - (b - 8), DC.MESH), (step, b + 8 - step, DC.MESH)]  # cut in two, nothing else
    elif stretch == STRETCHES[1]:  # an unmoved MESH head swallows SKINNED pairs of other full keys - up to the batch's end; behind it each is a head
        q.add(DC.MASKED, DC.val(5, DC.MESH))
        for k in range(15):
            q.add(DC.FULL, DC.val(k, DC.SKINNED, k & 1))
        want = [(b - 8, step - (b - 8), DC.MESH)] + [(i, 1, DC.SKINNED) for i in range(step, b + 8)]
    else:  # every pair a run of its own on both sides; the moved MESH pair of their key behind them is a head (no head in front of it took it)
        q.add(DC.MASKED, DC.val(3, DC.AUTO))
        for k in range(15):
            q.add(DC.SAME, DC.val((3, 5, 4)[k % 3], DC.AUTO))
        q.add(DC.SAME, DC.val(20, DC.MESH))
        want = [(i, 1, DC.AUTO) for i in range(b - 8, b + 8)] + [(b + 8, 1, DC.MOVED)]
    end = q.n
    q.run(n - q.n, DC.MESH, range(16, 32))
    keys, values = q.arrays()
    name = f"batch start at pair {step}, seam at {b}, {stretch}"
    go, gv = DC.instancer()
    runs, data, oracle = encode(scene, name, keys, values, 3, go, gv)
    got = DC.runs_in(runs, b - 8, end)
    assert got == want, f"{name}: runs {got}, the walk gives {want}"
    check_tiling(name, runs, n)
    assert_equal_bytes(scene[0], oracle, name)


@pytest.mark.parametrize("n", [DC.ROUND, DC.ROUND - 1])
@pytest.mark.parametrize("i", [4, 8, 10], ids=lambda i: DC.STATE_NAME[DC.ROUND_SITUATIONS[i][0]])
def test_sequence_ends_on_the_round_seam(scene, i, n):
    """n = 65 536: pair n would be the first of a new tile and a new round - the `i == d.n` stores of k_draw_heads, k_draw_run_starts and
    k_draw_runs land there, in a block of their own; n = 65 535: in the last lane of the last tile."""
    keys, values, windows, filler = DC.round_sequence(i)
    keys, values = keys[:n], values[:n]
    name = f"{n} pairs, {DC.STATE_NAME[DC.ROUND_SITUATIONS[i][0]]} behind the last"
    for n_batches in (1, 8):
        runs, data, want = encode(scene, name, keys, values, n_batches)
        check_tiling(name, runs, n)
        DC.check_windows(name, runs, [], [(f[0], min(f[1], n - f[0])) + f[2:] for f in filler if f[0] < n], n, n_batches)
        assert_equal_bytes(scene[0], want, f"{name}, {n_batches} batches")


def rel_pos(tr, e):
    return (tr["pos"][e] - np.array([3.0, -2.0, 7.5])).astype(np.float32).view(np.uint32)  # DC.view()'s camera


def test_runs_that_own_whole_tiles(scene):
    tr = scene[1][3]
    q = DC.Seq()
    want = [q.run(257, DC.MESH, range(16, 32)) + (DC.MOVED,)]
    want.append(q.run(3 * 256 + 1, DC.MESH, range(16), 1, split=True) + (DC.MESH,))  # from a tile's second lane: two tiles without a break, one with a full-key break only
    want.append(q.run(1280 - q.n, DC.SKINNED, range(32), 1) + (DC.SKINNED,))  # ends on a tile seam ...
    want.append(q.run(192, DC.MESH, range(17, 32), bucket=1) + (DC.MOVED,))  # ... the next run starts on it and ends on a wave seam
    de, d_front = DC.mixed_decal_entities(3 * 256 + 5, seed=11)
    want.append(q.run(len(de), DC.DECAL, de) + (DC.DECAL,))  # ... where a decal run starts
    ce, c_front = DC.mixed_decal_entities(3 * 256 + 5, seed=12)
    want.append(q.run(len(ce), DC.CURVE, ce, bucket=DC.DEPTH) + (DC.CURVE,))
    want.append(q.run(3, DC.MESH, range(16)) + (DC.MESH,))
    assert [w[0] for w in want[1:5]] == [257, 1026, 1280, 1472] and 0 < d_front < len(de) and 0 < c_front < len(ce)
    keys, values = q.arrays()
    runs, data, oracle = encode(scene, "whole tiles", keys, values, 1)
    assert DC.runs_in(runs, 0, q.n) == want
    assert [int(r["front_count"]) for r in runs[4:6]] == [d_front, c_front]
    for r, ents, words in ((runs[4], de, 13), (runs[5], ce, 17)):  # the front part upwards in walk order, the back part downwards from the slice's end
        rec = data[int(r["data_offset"]): int(r["data_offset"]) + len(ents) * 4 * words].view(np.uint32).reshape(len(ents), words)
        order = np.concatenate([ents[ents < 8], ents[ents >= 8][::-1]])
        place = np.flatnonzero((rec[:, 0:3] != np.stack([rel_pos(tr, e) for e in order])).any(axis=1))
        assert not len(place), f"kind {r['kind']}: record {place[0]} of {len(ents)} is not entity {order[place[0]]}'s"
    assert_equal_bytes(scene[0], oracle, "whole tiles")


def test_one_run_longer_than_a_round(scene):
    q = DC.Seq()
    want = [q.run(255, DC.MESH, range(16, 32), 1) + (DC.MOVED,), q.run(DC.ROUND + 257, DC.MESH, range(16), split=True) + (DC.MESH,), q.run(37, DC.SKINNED, range(32)) + (DC.SKINNED,)]
    keys, values = q.arrays()
    runs, data, oracle = encode(scene, "a run longer than a round", keys, values, 1)
    assert DC.runs_in(runs, 0, q.n) == want
    assert_equal_bytes(scene[0], oracle, "a run longer than a round")


def csr(sizes, seed):
    rng = np.random.default_rng(seed)
    go = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    gv = rng.integers(0, DC.N_ENTITIES, size=int(go[-1])).astype(np.uint64) | (rng.integers(0, 2, size=int(go[-1])).astype(np.uint64) << np.uint64(40))
    return go, gv


# group sizes -> edges at renderables 255, 256 and 257 (the last lane of k_draw_groups' first block, the first two of the second); empty
# groups first, last and three in a row; one group larger than a tile
CSRS = {"edges at 255, 256, 257": [0, 255, 1, 1, 0, 0, 0, 300, 43, 0], "one group": [300], "one group, a tile and one": [257], "one empty group": [0],
        "empty groups around a tile": [0, 0, 256, 0, 0, 0, 256, 1, 0]}


@pytest.mark.parametrize("name", list(CSRS))
def test_instancer_groups_around_a_tile_edge(scene, name):
    sizes = CSRS[name]
    go, gv = csr(sizes, seed=len(sizes))
    n_groups = len(sizes)
    named = sorted(set(range(n_groups)) | {n_groups, n_groups + 1, 200})  # every group, empty ones included, and indices at and behind n_groups
    q = DC.Seq()
    q.run(5, DC.MESH, range(16))
    for g in named:
        q.add(DC.MASKED, DC.val(g, DC.AUTO))
    q.run(3, DC.SKINNED, range(32))
    keys, values = q.arrays()
    runs, data, oracle = encode(scene, name, keys, values, 2, go, gv)
    auto = runs[runs["kind"] == DC.AUTO]
    assert [int(g) for g in auto["group"]] == named
    for r in auto:
        g = int(r["group"])
        frm, to = (int(go[g]), int(go[g + 1])) if g < n_groups else (0, 0)
        first = int(gv[frm]) if to > frm else 0
        got = tuple(int(r[f]) for f in ("pair_count", "total_count", "data_offset", "stride", "head_entity", "mesh_idx"))
        assert got == (1, to - frm, 48 * frm, 48, first & 0xFFFFFFFF, first >> 40), f"{name}: AUTOINSTANCED run of group {g}: {r}"
    assert_equal_bytes(scene[0], oracle, name)
