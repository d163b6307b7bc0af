"""Hand-made pair sequences for createCommands (renderer/pipeline.cpp:2747-3320) with the run boundaries the reference's walk gives them,
derived by hand from the while loops of each case. Shared by tests/test_draw_commands.py (the numpy oracle) and
tests/test_gpu_draw_commands.py (the device, through lmx_draw_run_pairs). Below them: built sequences that carry a chosen state of the
device's scan across its wave, tile and round edges (tests/test_gpu_draw_boundaries.py)."""
import numpy as np

from lumixengine_amd import api

MESH, AUTO, SKINNED, DECAL, CURVE, MOVED = 0, 1, 2, 3, 4, 32
N_ENTITIES = 32  # entities 16.. carry ModelInstance::MOVED
PLAIN, DEPTH = 0, 2  # buckets: 0 sorts by mesh key, 2 by depth


def key(bucket, low):
    return (bucket << 56) | low


def val(entity, type_, mesh_idx=0):
    return entity | (type_ << 32) | (mesh_idx << 40)


def tables():
    """(keys_scene-like dict, draw_tables-like dict, lod, transforms) over N_ENTITIES entities of one two-mesh model."""
    rng = np.random.default_rng(4)
    n = N_ENTITIES
    models = np.zeros(1, api.KEYS_MODEL)
    models["lod_distances"][0] = np.finfo(np.float32).max
    models["lod_indices"][0]["from"], models["lod_indices"][0]["to"] = 0, -1
    models["lod_indices"][0][0] = (0, 1)
    models["first_mesh"][0], models["mesh_count"][0] = 0, 2
    mm = np.zeros(2 * n, api.MESH_MATERIAL)
    mm["sort_key"] = np.arange(2 * n) % 7
    sc = {"models": models, "mesh_types": np.array([0, 1], np.uint8), "model": np.zeros(n, np.int32), "material_offset": (2 * np.arange(n)).astype(np.uint32),
          "mesh_materials": mm, "lod": rng.integers(0, 5, size=n).astype(np.float32), "flags": ((np.arange(n) >= 16) * 8 | 6).astype(np.uint8),
          "dirty": np.zeros(n, np.uint8), "pose_frame": np.zeros(n, np.uint32)}
    from lumixengine_amd import scenes

    dt = scenes.draw_tables(sc, n, seed=5, extent=50.0)
    dt["half_extents"][:] = 1.0
    dt["curve_half_extents"][:] = (0.5, 2.0, 1.0)
    tr = scenes.random_transforms(rng, n, 50.0)
    # the near plane of frustum() is z = 0: entities 0..7 lie far in front of it, 8..15 inside a decal's reach of it
    tr["pos"][:8, 2] = 100.0 + np.arange(8)
    tr["pos"][8:16, 2] = np.linspace(-1.5, 1.5, 8)
    return sc, dt, sc["lod"].copy(), tr


def frustum():
    fr = np.zeros(1, api.SHIFTED_FRUSTUM)
    fr["zs"][0, 0] = 1.0  # NEAR plane: distance = z
    return fr


def view(camera_pos=(3.0, -2.0, 7.5)):
    return api.draw_view(camera_pos=camera_pos, frustum=frustum(), bucket_depth_sorted=[0, 0, 1, 1])


K = 0x0000_0012_0000_0000  # a mesh key's place in a plain bucket's mask (bits 32..55 + bucket)

# name -> (pairs [(key, value)], n_batches, expected runs [(first, count, kind)])
CASES = {
    "batch boundary inside an equal-key stretch": ([(key(PLAIN, K), val(e, MESH)) for e in range(6)], 2, [(0, 3, MESH), (3, 3, MESH)]),
    "depth bucket, equal low 24 key bits": (
        [(key(DEPTH, (1 << 24) | 0x123456), val(0, MESH)), (key(DEPTH, (2 << 24) | 0x123456), val(1, MESH)), (key(DEPTH, (3 << 24) | 0x123457), val(2, MESH))], 1,
        [(0, 2, MESH), (2, 1, MESH)]),
    "SKINNED head swallows a MESH pair of its key": (
        [(key(PLAIN, K), val(1, SKINNED, 1)), (key(PLAIN, K), val(2, MESH)), (key(PLAIN, K + (1 << 32)), val(3, MESH))], 1, [(0, 2, SKINNED), (2, 1, MESH)]),
    "MESH head swallows SKINNED pairs of its masked key": (
        [(key(PLAIN, K), val(1, MESH)), (key(PLAIN, K), val(2, SKINNED, 1)), (key(PLAIN, K + 5), val(3, SKINNED, 1))], 1, [(0, 3, MESH)]),
    "unmoved MESH head in the middle of a masked segment": (
        [(key(PLAIN, K), val(1, SKINNED, 1)), (key(PLAIN, K + 1), val(2, MESH, 1)), (key(PLAIN, K + 2), val(3, SKINNED, 1)), (key(PLAIN, K + 3), val(9, DECAL)),
         (key(PLAIN, K + (1 << 32)), val(4, SKINNED, 1))], 1, [(0, 1, SKINNED), (1, 3, MESH), (4, 1, SKINNED)]),
    "moved MESH heads end at full-key breaks": (
        [(key(PLAIN, K), val(16, MESH)), (key(PLAIN, K), val(1, MESH)), (key(PLAIN, K + 1), val(17, MESH)), (key(PLAIN, K + 2), val(2, MESH)), (key(PLAIN, K + 3), val(18, MESH))], 1,
        [(0, 2, MOVED), (2, 1, MOVED), (3, 2, MESH)]),
    "AUTOINSTANCED swallowed between equal keys": (
        [(key(PLAIN, K), val(16, MESH)), (key(PLAIN, K), val(3, AUTO)), (key(PLAIN, K), val(17, MESH))], 1, [(0, 3, MOVED)]),
    "AUTOINSTANCED heads take one pair": (
        [(key(PLAIN, K), val(3, AUTO)), (key(PLAIN, K), val(4, AUTO)), (key(PLAIN, K), val(16, MESH)), (key(PLAIN, K), val(17, MESH)), (key(PLAIN, K), val(5, AUTO))], 1,
        [(0, 1, AUTO), (1, 1, AUTO), (2, 3, MOVED)]),
    "decal run, all front": ([(key(PLAIN, 77), val(e, DECAL)) for e in (0, 1, 2, 3)], 1, [(0, 4, DECAL)]),
    "decal run, all back": ([(key(PLAIN, 77), val(e, DECAL)) for e in (11, 12)], 1, [(0, 2, DECAL)]),
    "decal run, mixed": ([(key(PLAIN, 77), val(e, DECAL)) for e in (0, 11, 1, 12, 8, 2)] + [(key(PLAIN, 78), val(e, CURVE)) for e in (12, 3, 15, 11)], 1,
                         [(0, 6, DECAL), (6, 4, CURVE)]),
    "n not divisible by n_batches": ([(key(PLAIN, K + (k // 2 << 32)), val(k, MESH)) for k in range(7)], 3, [(0, 2, MESH), (2, 1, MESH), (3, 1, MESH), (4, 2, MESH), (6, 1, MESH)]),
    "n < n_batches": ([(key(PLAIN, K), val(0, MESH)), (key(PLAIN, K), val(1, MESH))], 8, [(0, 1, MESH), (1, 1, MESH)]),
    "a pair type the key run never emits": (
        [(key(PLAIN, K), val(1, 16)), (key(PLAIN, K), val(2, 16)), (key(PLAIN, K), val(3, MESH)), (key(PLAIN, K), val(4, 7))], 1, [(0, 1, 16), (1, 1, 16), (2, 2, MESH)]),
    "n = 0": ([], 4, []),
}


def instancer():
    """An instancer CSR for the AUTOINSTANCED pairs above (their value's low bits name the group): groups 3 and 5 hold renderables, 4 is empty."""
    offsets = np.array([0, 0, 0, 0, 3, 3, 7, 7], np.uint32)
    values = np.array([val(6, 0, 1), val(20, 0, 0), val(7, 0, 1), val(2, 0, 0), val(21, 0, 1), val(9, 0, 0), val(30, 0, 0)], np.uint64)
    return offsets, values


def arrays(name):
    pairs, n_batches, runs = CASES[name]
    keys = np.array([p[0] for p in pairs], np.uint64)
    values = np.array([p[1] for p in pairs], np.uint64)
    assert np.all(keys[1:] >= keys[:-1]), name
    return keys, values, n_batches, runs


# ---- Sequences that put a chosen scan state on a chosen pair ----------------------------------------------------------------------------
# draw_kernels.hip composes the pairs' steps on the state {streak, blocked} inside a wave (64 pairs), across the waves of a tile (256 pairs)
# and across tiles in rounds of 256 tiles (65 536 pairs). A "situation" is (state carried into pair b, key class of b against b - 1, kind of
# b); seam_sequence() builds sorted pairs in which pair b meets it, and the runs the reference's walk cuts around b - derived from the while
# loops of the walk, per situation, in _window() below (no state machine).
SAME, FULL, MASKED = 0, 1, 2  # the key of b: equal to b - 1's | a full-key break inside the masked segment | a masked-key break
ONE, UNMOVED, OTHER = 0, 1, 2  # b is: a one-pair head (AUTOINSTANCED, unknown type) | an unmoved MESH | moved MESH, SKINNED, DECAL, CURVE_DECAL
SITUATIONS = [(s, c, k) for s in range(4) for c in (SAME, FULL, MASKED) for k in (ONE, UNMOVED, OTHER)]  # 36
CLASS_NAME = ("with the key of the pair before", "behind a full-key break", "behind a masked-key break")
KIND_NAME = ("a one-pair head", "an unmoved MESH pair", "a moved MESH / SKINNED / decal pair")
STATE_NAME = ("state 0", "streak", "blocked", "blocked + streak")
FRONT_ENTITIES, BACK_ENTITIES = tuple(range(8)), (11, 12, 13, 14, 15)  # tables(): decals in front of the near plane / reaching it
BIG_DECAL = 4 * 256 + 5  # a filler decal run: three whole tiles inside it wherever it starts


def situation_name(s, c, k):
    return f"{STATE_NAME[s]} carried onto {KIND_NAME[k]} {CLASS_NAME[c]}"


def run_kind(value):
    """the kind of the run a pair heads"""
    t, e = (int(value) >> 32) & 31, int(value) & 0xFFFFFFFF
    return (MOVED if e >= 16 else MESH) if t == MESH else t


class Seq:
    """Sorted pairs, appended in order. Plain buckets (0, 1): masked key = bits 32..55, full-key breaks count up bits 0..31; depth-sorted
    buckets (2, 3): masked key = bits 0..23, every break counts up bits 24..55 (so the keys ascend) and a masked break changes bits 0..23 too."""

    def __init__(self):
        self.k, self.v, self.n = [], [], 0
        self.bucket, self.seg, self.sub = 0, 0, 0

    def _key(self, cls, bucket):
        if bucket is not None and bucket != self.bucket:
            assert bucket > self.bucket and cls == MASKED
            self.bucket, self.seg, self.sub = bucket, 0, 0
        elif cls == MASKED:
            self.seg += 1
            self.sub = self.sub + 1 if self.bucket >= DEPTH else 0
        elif cls == FULL:
            self.sub += 1
        assert self.seg < (1 << 24) - 1 and self.sub < (1 << 31)
        return key(self.bucket, (self.sub << 24) | self.seg) if self.bucket >= DEPTH else key(self.bucket, ((self.seg + 1) << 32) | self.sub)

    def add(self, cls, value, bucket=None):
        """one pair; -> its position"""
        self.k.append(np.array([self._key(cls, bucket)], np.uint64))
        self.v.append(np.array([value], np.uint64))
        self.n += 1
        return self.n - 1

    def extend(self, values):
        """pairs of the key of the pair in front of them"""
        values = np.asarray(values, np.uint64)
        self.k.append(np.full(len(values), self._key(SAME, None), np.uint64))
        self.v.append(values)
        self.n += len(values)

    def run(self, count, type_, entities, mesh_idx=0, bucket=None, split=False):
        """`count` pairs of one masked key behind a masked-key break, the entities cycling; split: a full-key break half way. -> (first, count)"""
        if count <= 0:
            return self.n, 0
        k0 = self._key(MASKED, bucket)
        keys = np.full(count, k0, np.uint64)
        if split and count > 1:
            keys[count // 2:] = self._key(FULL, None)
        e = np.asarray(entities, np.uint64)[np.arange(count) % len(entities)]
        self.k.append(keys)
        self.v.append(e | np.uint64((type_ << 32) | (mesh_idx << 40)))
        self.n += count
        return self.n - count, count

    def arrays(self):
        keys = np.concatenate(self.k) if self.k else np.zeros(0, np.uint64)
        values = np.concatenate(self.v) if self.v else np.zeros(0, np.uint64)
        assert np.all(keys[1:] >= keys[:-1])
        return keys, values


def mixed_decal_entities(count, seed):
    """front and back decal entities interleaved irregularly; -> (entities, how many lie in front)"""
    rng = np.random.default_rng(seed)
    e = np.array(FRONT_ENTITIES + BACK_ENTITIES)[rng.integers(0, 13, size=count)]
    e[:4] = (0, 11, 12, 1)
    return e, int((e < 8).sum())


def _fill(q, gap, bucket, pending, runs):
    """`gap` filler pairs in a few long runs: the pending big DECAL / CURVE_DECAL runs where they fit, a moved MESH run of an odd count
    (96-byte records: 16-byte copies from slices at every alignment), the rest one unmoved MESH run (two full keys)."""
    turn = len(runs)
    while pending and gap >= BIG_DECAL + 2:
        type_ = pending.pop(0)
        e, front = mixed_decal_entities(BIG_DECAL, seed=type_)
        first, count = q.run(BIG_DECAL, type_, e, bucket=bucket)
        runs.append((first, count, type_, front))
        gap -= BIG_DECAL
        bucket = None
    if gap >= 4:
        m = min((gap // 3) | 1, 1001)
        first, count = q.run(m, MESH, range(16 + turn % 5, 32), turn & 1, bucket=bucket)
        runs.append((first, count, MOVED, count))
        gap -= m
        bucket = None
    if gap > 0:
        first, count = q.run(gap, MESH, range(turn % 7, 16), (turn >> 1) & 1, bucket=bucket, split=True)
        runs.append((first, count, MESH, count))


ONES = (val(3, AUTO), val(2, 16), val(5, AUTO), val(6, 7), val(4, AUTO), val(9, AUTO))  # groups of instancer(): 3, 5 hold renderables, 4 is empty, 9 does not exist
OTHERS = (val(17, MESH, 1), val(5, SKINNED, 1), val(2, DECAL), val(12, CURVE), val(30, MESH), val(21, SKINNED), val(11, DECAL), val(3, CURVE))
UNMOVEDS = (val(1, MESH), val(9, MESH, 1), val(14, MESH), val(6, MESH, 1))


def _window(q, turn, s, c, k, b, hold=0):
    """Appends the prefix that leaves state s behind pair b - 1, the pair at b and two pairs of its masked segment; -> the runs of the
    reference's walk from the prefix's first pair (a masked-key break: a head whatever came before) to the filler behind (again one).
    hold: that many pairs of the prefix's last key between it and b which leave the state as it is - one-pair heads where it has a streak,
    pairs the running head swallows where it has none - so that the state crosses every seam in between."""
    one, other, unmoved = ONES[turn % len(ONES)], OTHERS[turn % len(OTHERS)], UNMOVEDS[turn % len(UNMOVEDS)]
    runs = []
    # the head whose while loop is running when the walk reaches b, and what ends that loop
    if s == 0:  # a moved MESH / SKINNED head: `while (sort_keys[i] == key)`
        assert q.n == b - 1 - hold
        head_value = OTHERS[(turn + 3) % len(OTHERS) & ~2]  # entries 0, 1, 4, 5: moved MESH and SKINNED
        head, rule = q.add(MASKED, head_value), FULL
    elif s == 1:  # a one-pair head, behind a masked-key break or behind a full-key break inside a moved head's segment
        if turn & 1:
            assert q.n == b - 2 - hold
            runs.append((q.add(MASKED, val(16 + turn % 16, MESH)), 1, MOVED))
        assert q.n == b - 1 - hold
        head_value = one
        head, rule = q.add(FULL if turn & 1 else MASKED, one), None
        if hold:  # a row of one-pair heads of one key
            held = np.array(ONES)[(np.arange(hold) + turn) % len(ONES)]
            runs += [(head, 1, run_kind(one))] + [(head + 1 + j, 1, run_kind(held[j])) for j in range(hold - 1)]
            q.extend(held)
            head, head_value = b - 1, held[-1]
    else:  # an unmoved MESH head: `while ((sort_keys[i] & instance_key_mask) == key)`; s == 3: an AUTOINSTANCED pair of another full key inside it
        assert q.n == b - (2 if s == 3 else 1) - hold
        head_value = UNMOVEDS[(turn + 1) % len(UNMOVEDS)]
        head, rule = q.add(MASKED, head_value), MASKED
        if s == 3:
            q.add(FULL, ONES[(turn + 1) % len(ONES) & ~1])  # entries 0, 2, 4: AUTOINSTANCED
            q.extend(np.array(ONES)[(np.arange(hold) + turn) % len(ONES) & ~1])
    if hold and s in (0, 2):  # swallowed whatever their type
        q.extend(np.array(UNMOVEDS + OTHERS + ONES[:2])[(np.arange(hold) + turn) % 14])
    head_kind = run_kind(head_value)
    value = (one, unmoved, other)[k]
    assert q.add(c, value) == b
    t1 = q.add(SAME, val(16 + (turn + 5) % 16, MESH, turn & 1))  # b's full key: a head only if b was a one-pair head
    t2 = q.add(FULL, val(16 + (turn + 9) % 16, MESH))  # b's masked key: a head unless an unmoved MESH head is still running
    end = t2 + 1
    is_head = rule is None or c >= rule  # the running loop ends at b: a one-pair head, or a break of the kind that loop compares
    if not is_head:
        if rule == MASKED:
            return runs + [(head, end - head, head_kind)]
        return runs + [(head, t1 + 1 - head, head_kind), (t2, 1, MOVED)]
    runs.append((head, b - head, head_kind))
    if k == ONE:
        return runs + [(b, 1, run_kind(value)), (t1, 1, MOVED), (t2, 1, MOVED)]
    if k == UNMOVED:
        return runs + [(b, 3, MESH)]
    return runs + [(b, 2, run_kind(value)), (t2, 1, MOVED)]


def seam_sequence(placed, n, buckets=None):
    """placed: [(position b, carried state s, (key class, kind) of the pair at b[, hold])], ascending and at least 6 apart; n: pairs in all.
    buckets: the bucket of each placed situation (ascending; default PLAIN).
    -> keys, values, windows [(b, s, c, k, first pair of the window, its end, runs [(first, count, kind)])], filler runs [(first, count,
    kind, front_count)]. The sequence carries one big DECAL and one big CURVE_DECAL filler run, so some gap has to leave them room."""
    q, windows, filler, pending = Seq(), [], [], [DECAL, CURVE]
    for turn, (b, s, (c, k), *hold) in enumerate(placed):
        hold = hold[0] if hold else 0
        bucket = PLAIN if buckets is None else buckets[turn]
        start = b - (2 if s == 3 or (s == 1 and turn & 1) else 1) - hold
        assert start >= q.n + (1 if bucket != q.bucket else 0), (b, q.n)  # room for the masked-key break a new bucket needs
        _fill(q, start - q.n, bucket, pending, filler)
        runs = _window(q, turn, s, c, k, b, hold)
        windows.append((b, s, c, k, start, q.n, runs))
    assert n >= q.n
    _fill(q, n - q.n, None, pending, filler)
    assert not pending, "no gap took the big decal runs"
    keys, values = q.arrays()
    assert len(keys) == n
    return keys, values, windows, filler


def wave_seams(first, count):
    """`count` positions b >= first with b % 64 == 0 and b % 256 != 0"""
    out, b = [], (first + 63) // 64 * 64
    while len(out) < count:
        if b % 256:
            out.append(b)
        b += 64
    return out


def _buckets(count):
    return [4 * i // count for i in range(count)]  # ascending over the buckets 0..3: plain, plain, depth-sorted, depth-sorted


# pair counts 8 * (64 j + 8): with n_batches = 8 the slice starts lie 8, 16, .. 56 pairs behind a wave edge, outside every window
WAVE_N, TILE_N = 8 * (64 * 11 + 8), 8 * (64 * 24 + 8)


def wave_sequence(shift=0):
    """all 36 situations, one per wave edge (shift: the whole layout moved by that many pairs)"""
    at = wave_seams(BIG_DECAL + 64, 36)
    return seam_sequence([(b + shift, s, (c, k)) for b, (s, c, k) in zip(at, SITUATIONS)], WAVE_N, _buckets(36))


def tile_sequence(shift=0):
    """all 36 situations, one per tile edge; rotated by half against wave_sequence(): every situation meets a plain and a depth-sorted bucket"""
    sit = SITUATIONS[18:] + SITUATIONS[:18]
    return seam_sequence([(256 * (6 + i) + shift, s, (c, k)) for i, (s, c, k) in enumerate(sit)], TILE_N, _buckets(36))


ROUND = 65536
ROUND_SITUATIONS = [(s, c, (s + c) % 3) for s in range(4) for c in (SAME, FULL, MASKED)]  # 12: the pair's kind rotates over the three


def round_sequence(i, n=ROUND + 300):
    """situation i of ROUND_SITUATIONS on pair 65 536, the first of the tile scan's second round"""
    s, c, k = ROUND_SITUATIONS[i]
    return seam_sequence([(ROUND, s, (c, k))], n, [(PLAIN, DEPTH, 1, 3)[i % 4]])


CARRY_AT, CARRY_HOLD = ROUND + 256, 300


def carry_sequence(i, n=CARRY_AT + 300):
    """k_draw_tile_scan hands `carry` from one round of 256 tiles to the next. The state in front of pair 65 536 is still the first round's
    (tile_in[255]); the carry first reaches the state in front of pair 65 792, behind tile 256 - if that whole tile leaves the state as it
    is. Situation i of ROUND_SITUATIONS on pair 65 792, its carried state set up in front of pair 65 536 and held for 300 pairs."""
    s, c, k = ROUND_SITUATIONS[i]
    return seam_sequence([(CARRY_AT, s, (c, k), CARRY_HOLD)], n, [(DEPTH, PLAIN, 3, 1)[i % 4]])


def scan_trace(keys, values, depth_sorted=(0, 0, 1, 1), moved_from=16):
    """For coverage only, never for expected values: the state {streak, blocked} (streak | blocked << 1) in front of every pair of one
    batch, with the pair's key class and kind. -> [(state, class, kind)]"""
    out, streak, blocked = [], 0, 0
    for i in range(len(keys)):
        key_, t, e = int(keys[i]), (int(values[i]) >> 32) & 31, int(values[i]) & 0xFFFFFFFF
        mask = 0xFF00_0000_00FF_FFFF if depth_sorted[key_ >> 56] else 0xFFFF_FFFF_0000_0000
        prev = int(keys[i - 1]) if i else ~key_
        c = MASKED if (prev & mask) != (key_ & mask) else FULL if prev != key_ else SAME
        k = ONE if t == AUTO or t > CURVE else UNMOVED if t == MESH and e < moved_from else OTHER
        out.append((streak | blocked << 1, c, k))
        if c == MASKED:
            blocked = 0
        if c != SAME:
            streak = 1
        if streak and k != ONE:
            blocked |= k == UNMOVED
            streak = 0
    return out


# name -> builder of (keys, values, windows, filler runs); shared by the oracle's and the device's tests
SEAM_SEQUENCES = {"wave seams": wave_sequence, "wave seams, last lane": lambda: wave_sequence(-1), "wave seams, second lane": lambda: wave_sequence(1),
                  "tile seams": tile_sequence, "tile seams, last lane": lambda: tile_sequence(-1), "tile seams, second lane": lambda: tile_sequence(1)}
SEAM_SEQUENCES.update({f"round seam, {situation_name(*ROUND_SITUATIONS[i])}": (lambda i=i: round_sequence(i)) for i in range(12)})
SEAM_SEQUENCES.update({f"round carry, {situation_name(*ROUND_SITUATIONS[i])}": (lambda i=i: carry_sequence(i)) for i in range(12)})


def seam_class(b):
    """the coarsest seam of the scan in front of pair b: "round", "tile", "wave" or None"""
    return None if b == 0 or b % 64 else "wave" if b % 256 else "tile" if b % ROUND else "round"


def runs_in(run_list, first, end):
    """the (first, count, kind) of the runs that start in [first, end); run_list: DRAW_RUN records or the tuples of draw_oracle.walk"""
    if isinstance(run_list, np.ndarray):
        sel = run_list[(run_list["first_pair"] >= first) & (run_list["first_pair"] < end)]
        return [(int(r["first_pair"]), int(r["pair_count"]), int(r["kind"])) for r in sel]
    return [(int(r[0]), int(r[1]), int(r[2])) for r in run_list if first <= r[0] < end]


def check_windows(name, run_list, windows, filler, n, n_batches=1):
    """Every window's and every filler run's boundaries in `run_list`; a failure names the seam and the situation. With several batches no
    slice start may touch a window (the sequences' pair counts see to it); filler runs are cut at the slice starts."""
    step = max((n + n_batches - 1) // n_batches, 1)
    cuts = list(range(step, n, step))
    for b, s, c, k, first, end, want in windows:
        assert not any(first <= x <= end for x in cuts), (name, b, step)
        got = runs_in(run_list, first, end)
        near = lambda runs: [r for r in runs if r[0] >= b - 3]  # noqa: E731 (a held state's window is long)
        assert got == want, (f"{name}: {seam_class(b) or 'lane ' + str(b % 64)} seam in front of pair {b}: {situation_name(s, c, k)}: runs {near(got)}, the walk "
                             f"gives {near(want)}{'' if near(got) != near(want) else ' (they differ in front of pair %d)' % (b - 3)}")
    for first, count, kind, front in filler:
        edges = [first] + [x for x in cuts if first < x < first + count] + [first + count]
        want = [(a, z - a, kind) for a, z in zip(edges[:-1], edges[1:])]
        got = runs_in(run_list, first, first + count)
        if got != want:
            odd = min(set(r[0] for r in got) ^ set(r[0] for r in want), default=first)  # the first run start only one of the two has
            seam = odd - odd % 64 if odd - odd % 64 > first else first
            raise AssertionError(f"{name}: filler run of {count} pairs at pair {first} (kind {kind}): a run starts at pair {odd} in only one of the two, the last seam in "
                                 f"front of it: {seam_class(seam)} seam at pair {seam}{' (a batch start)' if seam in cuts else ''}: runs {got[:6]}, the walk gives {want[:6]}")
