"""WorldSync::edit (lumixengine_amd/host/world_sync.h) RUN: tests/cpp/run_world_sync_edit.cpp drives the adapter through staged writes,
batches of World::destroyEntity / createEntity / setParent and propagations the way mi355_plugin.cpp's module does; what the mirror holds
after every step is compared bit for bit with the oracle's world (and with api.World on the same script). Runs on the MI355X and under
`pytest -m gpu --hostsim`."""
import numpy as np
import pytest

from lumixengine_amd import api, scenes
from tests import adapters_run as A
from tests import helpers as H
from tests import world_edit_cases as WE

pytestmark = pytest.mark.gpu
EDIT, WRITE, PROPAGATE, DUMP, QUEUE = 1, 2, 3, 4, 5
CREATED, DESTROYED, REPARENTED = 0, 1, 2
A.DRIVERS.setdefault("run_world_sync_edit", (["world_sync.h", "world_edit_queue.h"], []))


def edit_record(destroy, create, create_tr, reparent, want=True):
    rp = np.array(reparent, np.int32).reshape(-1, 2)
    return (A.u32(EDIT, len(destroy)) + A.raw(destroy, np.int32) + A.u32(len(create)) + A.raw(create, np.int32) + A.raw(create_tr, api.TRANSFORM) + A.u32(len(rp))
            + A.raw(rp[:, 0], np.int32) + A.raw(rp[:, 1], np.int32) + A.u32(1 if want else 0))


def write_record(entity, tr, world_space):
    return A.u32(WRITE, len(entity)) + A.raw(entity, np.int32) + A.raw(tr, api.TRANSFORM) + A.raw(world_space, np.uint32)


def test_world_sync_edit_matches_the_oracle(gpu_ctx, live_oracle, tmp_path):
    A.library()
    h = WE.chains(9, 4, seed=31)
    par = h["parent"]
    n = len(par)
    hs = WE.Harness(gpu_ctx, live_oracle, h, n_reserve=3, ref_destroy=False)
    scenario = A.u32(n) + A.raw(hs.ow.get_transforms()[:n], api.TRANSFORM) + A.raw(hs.ow.get_local_transforms()[:n], api.TRANSFORM) + A.raw(par, np.int32)
    d = WE.Model(par).depth()
    roots = [int(e) for e in np.flatnonzero(par < 0)]
    leaves = [int(e) for e in np.flatnonzero(d == 3)]
    mids = [int(e) for e in np.flatnonzero(d == 1)]
    rng = np.random.default_rng(8)
    want = []  # per DUMP: (alive, parent, world, local, moved set or None)

    def dump(moved=None):
        nonlocal scenario
        scenario += A.u32(DUMP)
        hs.check_oracle(f"dump {len(want)}")
        want.append((hs.model.alive.copy(), hs.model.parent.copy(), hs.w.getTransforms(), hs.w.getLocalTransforms(), moved))

    def write(entity, world_space):
        nonlocal scenario
        entity = np.array(entity, np.int32)
        tr = scenes.random_transforms(rng, len(entity), 300.0)
        for i, e in enumerate(entity):  # (ancestors first in these scripts)
            (hs.ow.set_transforms if world_space[i] or hs.model.parent[e] < 0 else hs.ow.set_local_transforms)(entity[i : i + 1], tr[i : i + 1])
        ws = np.array(world_space, bool)
        hs.w.setTransforms(entity[~ws], tr[~ws])
        hs.w.setWorldTransforms(entity[ws], tr[ws])
        scenario += write_record(entity, tr, np.array(world_space, np.uint32))

    def edit(destroy=(), create=(), reparent=()):
        nonlocal scenario
        tr = scenes.random_transforms(rng, len(create), 500.0)
        hs.edit(destroy=destroy, create=create, create_tr=tr, reparent=reparent)
        scenario += edit_record(list(destroy), list(create), tr, list(reparent))

    hs.w.readMoved()
    # a write staged and not propagated, then a batch: the edit propagates it first, and its moved list stays readable
    write([roots[2]], [1])
    edit(destroy=[mids[0]], create=[n, n + 2], reparent=[(roots[1], leaves[4]), (n, roots[3]), (-1, mids[5])])
    dump(moved=set(hs.w.readMoved()[0].tolist()))
    # the index that died comes back in the same call as another dies; a child write and a root write behind it
    edit(destroy=[leaves[6]], create=[mids[0]], reparent=[(mids[0], leaves[7])])
    write([roots[0], leaves[7]], [0, 0])
    scenario += A.u32(PROPAGATE)
    hs.w.propagate()
    dump(moved=set(hs.w.readMoved()[0].tolist()))
    # a batch whose last entry closes a cycle is refused whole: nothing changes
    below = next(e for e in leaves if hs.model.alive[e] and hs.model.parent[e] >= 0 and hs.model.parent[hs.model.parent[e]] >= 0)
    top = int(hs.model.parent[hs.model.parent[below]])
    doomed = next(e for e in leaves if hs.model.alive[e] and not hs.model.is_ancestor(top, e))
    scenario += edit_record([doomed], [], np.zeros(0, api.TRANSFORM), [(below, top)], want=False)
    with pytest.raises(api.LumixError):
        hs.w.edit(destroy=[doomed], reparent=[(below, top)])
    dump(moved=set())

    out = A.run_driver("run_world_sync_edit", tmp_path, scenario)
    for k, (alive, parent, world, local, moved) in enumerate(want):
        got_world = out.counted(api.TRANSFORM)
        assert len(got_world) == len(alive), f"dump {k}: the adapter's range"
        got_local = out.arr(api.TRANSFORM, len(alive))
        got_moved = out.counted(np.int32)
        assert H.transforms_bits_equal(got_world[alive], world[alive]), f"dump {k}: world transforms"
        has_parent = alive & (parent >= 0)
        assert H.transforms_bits_equal(got_local[has_parent], local[has_parent]), f"dump {k}: stored locals"
        assert set(got_moved.tolist()) == moved, f"dump {k}: moved set"
    assert out.done()


def test_plugin_queue_folds_a_frame_into_the_batch(gpu_ctx, oracle_port, tmp_path):
    """WorldEditQueue (world_edit_queue.h, what Mi355Module queues entityCreated / entityDestroyed / setParent into): a frame of World calls -
    an entity created and destroyed again, one re-parented twice, a subtree destroyed children first and its root's index handed out
    again, an entity re-parented and then destroyed - reaches the mirror as the batch that states the frame's outcome."""
    A.library()
    h = WE.chains(8, 4, seed=33)
    par = h["parent"]
    n = len(par)
    hs = WE.Harness(gpu_ctx, oracle_port, h, n_reserve=2, ref_destroy=False)
    scenario = A.u32(n) + A.raw(hs.ow.get_transforms()[:n], api.TRANSFORM) + A.raw(hs.ow.get_local_transforms()[:n], api.TRANSFORM) + A.raw(par, np.int32)
    m = WE.Model(par)
    d = m.depth()
    roots = [int(e) for e in np.flatnonzero(par < 0)]
    leaves = [int(e) for e in np.flatnonzero(d == 3)]
    sub_root = int(np.flatnonzero(d == 1)[2])
    sub = m.subtree(sub_root)  # parents before children
    x, y = n, n + 1
    leaf = next(e for e in leaves if e not in sub)
    gone = next(e for e in leaves if e not in sub and e != leaf)
    events = [(CREATED, x), (REPARENTED, x), (CREATED, y), (REPARENTED, y), (DESTROYED, y), (REPARENTED, leaf), (REPARENTED, leaf)]
    events += [(DESTROYED, e) for e in reversed(sub)]  # destroyEntity announces the children first
    events += [(CREATED, sub_root), (REPARENTED, sub_root), (REPARENTED, gone), (DESTROYED, gone)]
    rng = np.random.default_rng(4)
    tr = scenes.random_transforms(rng, 2, 400.0)
    # the frame's outcome, as World's calls in batch order
    hs.edit(destroy=sub + [gone], create=[x, sub_root], create_tr=tr, reparent=[(roots[1], x), (roots[2], leaf), (roots[3], sub_root)])
    hs.check_oracle("the frame")
    after_tr = np.zeros(n + 2, api.TRANSFORM)
    after_tr[: n + 1] = hs.w.getTransforms()
    after_parent = np.full(n + 2, -1, np.int32)
    after_parent[: n + 1] = np.where(hs.model.alive, hs.model.parent, -1)
    valid = np.zeros(n + 2, np.uint32)
    valid[: n + 1] = hs.model.alive
    scenario += A.u32(QUEUE, len(events)) + b"".join(A.u32(k) + A.raw([e], np.int32) for k, e in events)
    scenario += A.u32(n + 2) + A.raw(after_tr, api.TRANSFORM) + A.raw(after_parent, np.int32) + A.raw(valid, np.uint32) + A.u32(1)
    scenario += A.u32(DUMP)
    live_roots = np.array([e for e in hs.model.live() if hs.model.parent[e] < 0], np.int32)
    moved = scenes.random_transforms(rng, len(live_roots), 900.0)
    first = (hs.w.getTransforms(), hs.w.getLocalTransforms())
    hs.ow.set_transforms(live_roots, moved)
    hs.w.setTransforms(live_roots, moved)
    hs.w.propagate()
    hs.check_oracle("after the root moves")
    scenario += write_record(live_roots, moved, np.ones(len(live_roots), np.uint32)) + A.u32(PROPAGATE, DUMP)
    out = A.run_driver("run_world_sync_edit", tmp_path, scenario)
    alive, has_parent = hs.model.alive, hs.model.alive & (hs.model.parent >= 0)
    for k, (world, local) in enumerate((first, (hs.w.getTransforms(), hs.w.getLocalTransforms()))):
        got_world = out.counted(api.TRANSFORM)
        assert len(got_world) == n + 1, "the range grew to the highest index that lives (the one created and destroyed again does not count)"
        got_local = out.arr(api.TRANSFORM, n + 1)
        out.counted(np.int32)
        assert H.transforms_bits_equal(got_world[alive], world[alive]), f"dump {k}: world transforms"
        assert H.transforms_bits_equal(got_local[has_parent], local[has_parent]), f"dump {k}: stored locals"
    assert out.done()


def test_queue_write_to_an_index_created_again_this_frame(gpu_ctx, oracle_port, tmp_path):
    """The World's free list hands a destroyed index straight back: createEntity, then a transform write to the new entity in the same
    frame, with other writes staged beside it. The mirror still holds the index as dead when the frame's batch is applied: the write
    must wait for the create instead of being refused, the batch must not fall back to a rebuild (apply returns true), and none of the
    frame's other writes may be lost."""
    A.library()
    h = WE.chains(6, 3, seed=35)
    par = h["parent"]
    n = len(par)
    hs = WE.Harness(gpu_ctx, oracle_port, h, ref_destroy=False)
    scenario = A.u32(n) + A.raw(hs.ow.get_transforms()[:n], api.TRANSFORM) + A.raw(hs.ow.get_local_transforms()[:n], api.TRANSFORM) + A.raw(par, np.int32)
    d = WE.Model(par).depth()
    roots = [int(e) for e in np.flatnonzero(par < 0)]
    back = int(np.flatnonzero(d == 2)[3])  # a leaf: dies in one frame, its index lives again in the next
    kid = int(np.flatnonzero(d == 1)[4])
    rng = np.random.default_rng(6)
    none = np.zeros(0, api.TRANSFORM)
    # frame 1: the entity dies
    hs.edit(destroy=[back])
    hs.w.propagate()
    scenario += edit_record([back], [], none, []) + A.u32(PROPAGATE)
    # frame 2: a root write and a child write, createEntity hands the index out again, the game writes the new entity's transform
    tr = scenes.random_transforms(rng, 4, 400.0)
    created_with, written = tr[2:3], tr[3:4]
    hs.ow.set_transforms(np.array([roots[1]], np.int32), tr[0:1])
    hs.ow.set_local_transforms(np.array([kid], np.int32), tr[1:2])
    hs.w.setTransforms([roots[1], kid], tr[0:2])
    scenario += write_record([roots[1], kid, back], np.concatenate([tr[0:2], written]), np.array([1, 0, 1], np.uint32))
    hs.edit(create=[back], create_tr=created_with)
    hs.ow.set_transforms(np.array([back], np.int32), written)
    hs.w.setWorldTransforms([back], written)
    hs.w.propagate()
    hs.check_oracle("the frame")
    after_tr = hs.w.getTransforms().copy()
    after_tr[back] = created_with[0]  # (the write went through the module: the World does not hold it)
    scenario += A.u32(QUEUE, 1) + A.u32(CREATED) + A.raw([back], np.int32)
    scenario += A.u32(n) + A.raw(after_tr, api.TRANSFORM) + A.raw(np.where(hs.model.alive, hs.model.parent, -1), np.int32) + A.raw(hs.model.alive, np.uint32) + A.u32(1)
    scenario += A.u32(PROPAGATE, DUMP)
    out = A.run_driver("run_world_sync_edit", tmp_path, scenario)
    got_world = out.counted(api.TRANSFORM)
    got_local = out.arr(api.TRANSFORM, n)
    out.counted(np.int32)
    assert hs.model.alive.all()
    assert H.transforms_bits_equal(got_world[back : back + 1], written), "the write to the entity created this frame"
    assert H.transforms_bits_equal(got_world, hs.w.getTransforms()), "world transforms: every write of the frame"
    has_parent = hs.model.parent >= 0
    assert H.transforms_bits_equal(got_local[has_parent], hs.w.getLocalTransforms()[has_parent]), "stored locals"
    assert out.done()
