"""The pose processor (pose_kernels.hip) on lists that span waves, tiles and blocks: the three levels of its prefix sum (lanes of a wave by
shuffle, the waves of a block through s_wave, the blocks through block_sum -> s_base with the carry from tile to tile), the counters added
by many blocks and the strided loop of the dual-quaternion waves. tests/test_gpu_pose_processor.py lists 40 entities at most: block 0's
first tile holds them all.

Every expectation is PO.pack (the CPU packing) and the oracle's computeSkeletonDualQuats of tests/pose_oracle.py's dense scene, compared
byte for byte; nothing is read from the device to be compared with the device. Every edge position is computed from api.POSE_BLOCK /
POSE_GRID / POSE_DQ_GRID (tests/test_pose_constants.py ties them to lmx_kernels.h). Each test has a context of its own."""
import numpy as np
import pytest

from lumixengine_amd import api
from tests import pose_oracle as PO
from tests.test_gpu_pose_processor import chain_scene

pytestmark = pytest.mark.gpu

WAVE = 64
N_DENSE_ENTITIES = 6000  # the entity table of the dense list and of the overflow test: the 4500 instances at scattered entities, the rest holes


def part_length(n):
    """A block's part of a list of n entries (pose_kernels.hip): whole tiles of POSE_BLOCK entries."""
    per = -(-n // api.POSE_GRID)
    return -(-per // api.POSE_BLOCK) * api.POSE_BLOCK


def dense_table():
    rng = np.random.default_rng(71)
    skinned = rng.choice(N_DENSE_ENTITIES, size=PO.N_DENSE, replace=False)
    table = np.full(N_DENSE_ENTITIES, -1, np.int32)
    table[skinned] = rng.permutation(PO.N_DENSE)
    return table, skinned


def preloaded(n, seed):
    """pose->slice values no pass writes (offsets are odd), uploaded through DrawCommands.setBones in front of a test"""
    rng = np.random.default_rng(seed)
    return rng.integers(1 << 24, 1 << 30, size=n).astype(np.uint32), (rng.integers(0, 1 << 16, size=n) * 32 + 1).astype(np.uint32)


def expected_tables(h0, o0, slices, handle, base):
    h, o = h0.copy(), o0.copy()
    for e, (off, _) in slices.items():
        h[e], o[e] = handle, base + off
    return h, o


def assert_tables(pp, want_h, want_o, what):
    h, o = pp.readSlices()
    bad = np.flatnonzero((h != want_h) | (o != want_o))
    assert len(bad) == 0, (f"{what}: pose->slice of {len(bad)} entities differ, the first: entity {bad[0]} has ({h[bad[0]]:#x}, {o[bad[0]]}), "
                           f"expected ({want_h[bad[0]]:#x}, {want_o[bad[0]]})")


def test_dense_list_every_block_level(oracle_port):
    sc, want_dq = PO.dense_scene(), PO.dense_dual_quats(oracle_port)
    bones = sc["bones"]
    table, skinned = dense_table()
    listed = np.random.default_rng(72).permutation(skinned).astype(np.int32)  # every lane of the blocks with work carries a non-zero, varying size
    n, per = len(listed), part_length(len(listed))
    assert n > api.POSE_DQ_GRID * (api.POSE_BLOCK // WAVE), "the dual-quaternion waves must take a second pass"
    assert n > 4 * per and n % per != 0, "several blocks with work, the last one partly filled"
    h0, o0 = preloaded(N_DENSE_ENTITIES, 73)
    handle, base = 0x00C0FFEE, 8192
    slices, total, skipped, overflow = PO.pack(listed, table, bones)
    assert len(slices) == n and total == PO.DUAL_QUAT_BYTES * int(bones.sum()) and (skipped, overflow) == (0, 0)
    ctx = api.Context(0)
    try:
        PO.upload_dense(api, ctx)
        api.DrawCommands(ctx).setBones(h0, o0)
        pp = api.PoseProcessor(ctx)
        pp.setInstances(table)
        pp.beginFrame(handle, base)
        pp.runList(listed)
        assert pp.counts() == {"instances": PO.N_DENSE, "bytes": total, "skipped": 0, "overflow": 0}  # the last slice ends at the buffer's last byte
        assert_tables(pp, *expected_tables(h0, o0, slices, handle, base), "dense list")  # entities not listed keep the preloaded values
        buf = pp.readBuffer()
        assert len(buf) == total
        PO.assert_slices_hold(buf, slices, want_dq, bones, "dense list")
        assert buf.tobytes() == b"".join(np.ascontiguousarray(want_dq[table[e]]).tobytes() for e in listed)  # back to back in list order
    finally:
        ctx.close()


N_LONG = 70_000  # entries of the sparse list and entities of its table
N_RANDOM_SKINNED = 2000


def long_list():
    """-> (list, table, skinned positions, edge positions). The skinned entries sit on every kind of edge of the slice steps and at
    N_RANDOM_SKINNED further positions; all others are holes of the four kinds, mixed."""
    n, per, n_inst = N_LONG, part_length(N_LONG), PO.N_DENSE
    last = (n - 1) // per  # the last block with work
    assert per >= 2 * api.POSE_BLOCK, "two tiles per block at least: the carry from tile to tile must be live"
    assert last >= 4 and n % per != 0, "several full blocks and a partial one"

    def edges(b):  # the tile edge inside block b and the edge between b and b + 1
        return [b * per + api.POSE_BLOCK - 1, b * per + api.POSE_BLOCK, (b + 1) * per - 1, (b + 1) * per]

    edge = {0, WAVE - 1, WAVE, *edges(0), *edges(last // 2), *edges(last - 1), last * per, n - 1}
    edge |= {p for p in (last * per + api.POSE_BLOCK - 1, last * per + api.POSE_BLOCK) if p < n}  # the partial block's own tile edge, where it has one
    assert all(0 <= p < n for p in edge)
    rng = np.random.default_rng(74)
    others = np.setdiff1d(np.arange(n), sorted(edge))
    at = np.sort(np.concatenate([sorted(edge), rng.choice(others, size=N_RANDOM_SKINNED, replace=False)])).astype(np.int64)
    k = len(at)
    assert k <= n_inst
    entity = rng.choice(N_LONG, size=k, replace=False)
    # the table: an instance each for the listed entities; of the others half have none, half one past the instance table
    table = np.where(rng.random(N_LONG) < 0.5, -1, n_inst + rng.integers(0, 1000, size=N_LONG)).astype(np.int32)
    table[rng.choice(np.flatnonzero(table >= n_inst), size=50, replace=False)] = np.iinfo(np.int32).max
    table[entity] = rng.choice(n_inst, size=k, replace=False)  # no instance twice
    unskinned = np.setdiff1d(np.arange(N_LONG), entity)
    none, past = unskinned[table[unskinned] < 0], unskinned[table[unskinned] >= n_inst]
    kind = rng.integers(0, 4, size=n)
    listed = np.select([kind == 0, kind == 1, kind == 2],
                       [np.full(n, -1), N_LONG + rng.integers(0, 1000, size=n), rng.choice(none, size=n)], rng.choice(past, size=n)).astype(np.int32)
    listed[rng.choice(np.flatnonzero(kind == 1), size=50, replace=False)] = np.iinfo(np.int32).max
    listed[at] = entity
    return listed, table, at, sorted(edge)


def test_sparse_long_list_tile_and_block_edges(oracle_port):
    sc, want_dq = PO.dense_scene(), PO.dense_dual_quats(oracle_port)
    bones = sc["bones"]
    listed, table, at, edge = long_list()
    n = len(listed)
    slices, total, skipped, overflow = PO.pack(listed, table, bones)
    assert len(slices) == len(at) and skipped == n - len(at) and overflow == 0 and all(int(listed[p]) in slices for p in edge)
    split = n // 2 + 37
    assert split % WAVE != 0
    s1, t1, k1, _ = PO.pack(listed[:split], table, bones)
    s2, t2, k2, _ = PO.pack(listed[split:], table, bones, start=t1)
    assert {**s1, **s2} == slices and t2 == total and min(off for off, _ in s2.values()) == t1 and len(s1) > api.POSE_BLOCK < len(s2)
    h0, o0 = preloaded(N_LONG, 75)
    ctx = api.Context(0)
    try:
        PO.upload_dense(api, ctx)
        api.DrawCommands(ctx).setBones(h0, o0)
        pp = api.PoseProcessor(ctx)
        pp.setInstances(table)
        handle, base = 0x0051DE, 1 << 16
        pp.beginFrame(handle, base)
        pp.runList(listed)
        assert pp.counts() == {"instances": len(at), "bytes": total, "skipped": n - len(at), "overflow": 0}
        want_h, want_o = expected_tables(h0, o0, slices, handle, base)
        assert_tables(pp, want_h, want_o, "one call")  # no entry but the listed ones' changed
        buf = pp.readBuffer()
        assert len(buf) == total
        PO.assert_slices_hold(buf, slices, want_dq, bones, "one call")
        # the same list in two calls: the second one's blocks all start from the cursor the first one left (POSES_BASE)
        handle, base = 0x0052DE, 1 << 20
        pp.beginFrame(handle, base)
        pp.runList(listed[:split])
        assert pp.counts() == {"instances": len(s1), "bytes": t1, "skipped": k1, "overflow": 0}
        assert_tables(pp, *expected_tables(want_h, want_o, s1, handle, base), "first of two calls")
        pp.runList(listed[split:])
        assert pp.counts() == {"instances": len(at), "bytes": total, "skipped": k1 + k2, "overflow": 0}
        assert_tables(pp, *expected_tables(want_h, want_o, slices, handle, base), "two calls")  # every slice where the one call put it
        PO.assert_slices_hold(pp.readBuffer(), slices, want_dq, bones, "two calls")
    finally:
        ctx.close()


def test_overflow_across_blocks(oracle_port):
    sc, want_dq = PO.dense_scene(), PO.dense_dual_quats(oracle_port)
    bones = sc["bones"]
    table, skinned = dense_table()
    capacity = PO.DUAL_QUAT_BYTES * int(bones.sum())
    first = np.random.default_rng(76).permutation(skinned)[:3000].astype(np.int32)
    second = np.random.default_rng(77).permutation(skinned).astype(np.int32)
    s1, t_first, _, ov1 = PO.pack(first, table, bones, capacity=capacity)
    s2, t2, _, ov2 = PO.pack(second, table, bones, start=t_first, capacity=capacity)
    # what the two permutations were chosen for, shown on the CPU: the second call's first entry that does not fit lies inside the list, is a
    # large skeleton that leaves room smaller ones behind it would fit into, and the refused entries span many blocks' parts
    refused = np.array([p for p, e in enumerate(second) if int(e) not in s2])
    sizes = PO.DUAL_QUAT_BYTES * bones[table[second]]
    room = capacity - t2
    assert len(s1) == 3000 and ov1 == 0 and ov2 == 1 and len(s2) >= 100 and len(refused) >= 1000
    assert len(set(refused // part_length(len(second)))) >= 4 and refused[0] % WAVE not in (0, WAVE - 1)
    assert 0 < room < sizes[refused[0]] and (sizes[refused[1:]] <= room).sum() >= 100
    h0, o0 = preloaded(N_DENSE_ENTITIES, 78)
    handle, base = 0x0F10, 512
    ctx = api.Context(0)
    try:
        PO.upload_dense(api, ctx)
        api.DrawCommands(ctx).setBones(h0, o0)
        pp = api.PoseProcessor(ctx)
        pp.setInstances(table)
        pp.beginFrame(handle, base)
        pp.runList(first)
        assert pp.counts() == {"instances": 3000, "bytes": t_first, "skipped": 0, "overflow": 0}
        h1, o1 = expected_tables(h0, o0, s1, handle, base)
        assert_tables(pp, h1, o1, "first call")
        pp.runList(second)
        assert pp.counts() == {"instances": 3000 + len(s2), "bytes": t2, "skipped": 0, "overflow": 1}
        assert_tables(pp, *expected_tables(h1, o1, s2, handle, base), "second call")  # a refused entity keeps what it had before this call
        buf = pp.readBuffer(capacity + api.POSES_GUARD_BYTES)
        assert (buf[capacity:] == 0xA5).all(), "written behind the buffer"
        PO.assert_slices_hold(buf, s1, want_dq, bones, "first call's slices")
        PO.assert_slices_hold(buf, s2, want_dq, bones, "accepted slices of the second call")
    finally:
        ctx.close()


def test_chain_with_more_than_one_block_of_visible_skeletons(oracle_port):
    want_dq = PO.dense_dual_quats(oracle_port)
    bones = PO.dense_scene()["bones"]
    n_skinned = 1500
    base, sc, dt, tr, table, skinned = chain_scene(n_mesh=3000, n_skinned=n_skinned, seed=81)  # the dense scene's first 1500 instances
    n = len(table)
    ctx = api.Context(0)
    try:
        PO.upload_dense(api, ctx)
        cs = api.CullingSystem(ctx)
        cs.build(base["entity"], np.zeros(n, np.uint8), tr["pos"], base["radius"])
        sk = api.SortKeys(ctx)
        sk.setModels(sc["models"], sc["mesh_types"])
        sk.setInstances(sc["model"], sc["material_offset"], sc["mesh_materials"], sc["lod"], sc["flags"], sc["dirty"], sc["pose_frame"])
        sk.setPositions(tr["pos"])
        dc = api.DrawCommands(ctx)
        dc.setMeshes(dt["mesh_lod"])
        dc.setMaterialIndices(dt["material_index"])
        dc.setTransforms(tr)
        dc.setPrevTransforms(dt["prev"])
        pp = api.PoseProcessor(ctx)
        pp.setInstances(table)
        cam = ((0.0, 0.0, 700.0), (0.0, 0.0, 0.0, 1.0))  # in front of the box, far enough to see most of it
        frustum = api.viewport_frustum(pos=cam[0], rot=cam[1], far=2000.0)
        handle, slice_base = 0x4321, 1024
        pp.beginFrame(handle, slice_base)
        cs.cull(frustum)
        sk.run(api.keys_view(camera_pos=cam[0], time_delta=1 / 60, frame_number=7, layer_to_bucket=sc["layer_to_bucket"], bucket_depth_sorted=sc["bucket_depth_sorted"]), 15)
        pp.run()  # the list and its length are on the device only
        poses = [int(e) for e in sk.readPoses()]
        assert 2 * api.POSE_BLOCK < len(poses) < n_skinned and len(set(poses)) == len(poses) and set(poses) <= skinned, len(poses)
        cnt = pp.counts()
        assert cnt["instances"] == len(poses) and cnt["skipped"] == 0 and cnt["overflow"] == 0
        assert cnt["bytes"] == PO.DUAL_QUAT_BYTES * int(bones[table[poses]].sum())
        h, o = pp.readSlices()
        owners = [int(e) for e in np.flatnonzero(h == handle)]
        assert set(owners) == set(poses)
        at = 0  # sorted by offset the slices tile [0, bytes): each starts where the one before it ends
        for e in sorted(owners, key=lambda e: int(o[e])):
            assert int(o[e]) == slice_base + at, f"entity {e}"
            at += PO.DUAL_QUAT_BYTES * int(bones[table[e]])
        assert at == cnt["bytes"]
        buf = pp.readBuffer()
        assert len(buf) == at
        PO.assert_slices_hold(buf, {e: (int(o[e]) - slice_base, int(table[e])) for e in owners}, want_dq, bones, "chain")
        # on to the draw records: words 1 and 2 of every skinned 92-byte record are its entity's pose->slice
        sk.sort()
        dc.run(api.draw_view(camera_pos=cam[0], frustum=frustum, bucket_depth_sorted=sc["bucket_depth_sorted"]), 1)
        _, values = sk.readPairs()
        data = dc.readInstanceData()
        seen = set()
        for r in dc.readRuns():
            if int(r["kind"]) != api.RUN_SKINNED:
                continue
            assert int(r["stride"]) == 92
            for j in range(int(r["pair_count"])):
                v = int(values[int(r["first_pair"]) + j])
                if (v >> 32) & 31 != api.RUN_SKINNED:
                    continue
                e = v & 0xFFFFFFFF
                w = data[int(r["data_offset"]) + 92 * j : int(r["data_offset"]) + 92 * (j + 1)].view(np.uint32)
                assert (int(w[1]), int(w[2])) == (handle, int(o[e])), f"skinned record of entity {e}"
                seen.add(e)
        assert seen == set(poses) == set(int(e) for e in cs.cull(frustum).ids(0, 0)) & skinned
    finally:
        ctx.close()
