"""lmx_world_edit: World::destroyEntity / createEntity / setParent for a batch, with the slot order derived again on the device.
Every script step is checked (a) against the oracle, (b) against a fresh build of the same hierarchy in a second context, and
(c) for identical bytes when the script runs twice. Needs an MI355X, or `-m gpu --hostsim`."""
import os

import numpy as np
import pytest

from lumixengine_amd import api, scenes
from tests import helpers as H
from tests import world_edit_cases as WE

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx2():
    """the context of the fresh builds of check (b)"""
    ctx = api.Context(0)
    yield ctx
    ctx.close()


def run_script(gpu_ctx, ctx2, oracle, h, steps, n_reserve=0, ref_destroy=True, fresh_every=1):
    """steps: callables (harness) -> dict for Harness.edit. Runs the script twice; returns the harness of the second run."""
    runs = []
    for rep in range(2):
        hs = WE.Harness(gpu_ctx, oracle, h, n_reserve=n_reserve, ref_destroy=ref_destroy)
        snaps = []
        for i, step in enumerate(steps):
            hs.edit(**step(hs))
            hs.check_oracle(f"step {i}")
            snaps.append(hs.snapshot())
            hs.write()
            hs.w.propagate()
            hs.check_oracle(f"step {i} after the writes")
            snaps.append(hs.snapshot())
            if (i % fresh_every == fresh_every - 1 or i + 1 == len(steps)):
                hs.check_fresh_build(ctx2, f"step {i}")
        runs.append(snaps)
    assert runs[0] == runs[1], "two runs of one script gave different bytes"  # (c)
    return hs


def seeded_steps(seed, n_total, count, recreate):
    rng = np.random.default_rng(seed)
    ever = np.zeros(n_total, bool)

    made = {}

    def step_at(i):
        def step(hs):
            if i not in made:  # (the second run of the script replays the first one's batches)
                ever[: hs.model.n] |= hs.model.alive
                d, c, r = WE.random_batch(rng, hs.model, n_total, recreate=recreate, ever_created=ever)
                made[i] = {"destroy": d, "create": c, "reparent": r}
            return made[i]

        return step

    return [step_at(i) for i in range(count)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_world_sizes(gpu_ctx, ctx2, live_oracle, n):
    """one wave, its edges, a block's edge (the one-block level expansion ends at 256 slots), a second scan tile"""
    h = WE.forest(n, seed=n)
    recreate = live_oracle.kind != "reference"
    run_script(gpu_ctx, ctx2, live_oracle, h, seeded_steps(100 + n, n + 6, 4, recreate), n_reserve=6, ref_destroy=not recreate)


@pytest.mark.parametrize("flat", [257, 1025])
def test_world_wide_levels(gpu_ctx, ctx2, oracle_port, flat):
    """every level wider than the one-block expansion: chains, so that levels 0..2 all hold `flat` slots"""
    h = WE.chains(flat, 3, seed=5)
    n = len(h["parent"])
    steps = [lambda hs: {"reparent": [(1, 0), (0 + flat, 2), (-1, n - 1)]}, lambda hs: {"destroy": [1], "create": [n + 3]},
             lambda hs: {"create": [0], "reparent": [(n + 3, 0), (0, 5)]}]
    run_script(gpu_ctx, ctx2, oracle_port, h, steps, n_reserve=4, ref_destroy=False)


@pytest.mark.parametrize("depth", [1, 2, 16, 17])
def test_world_depths(gpu_ctx, ctx2, oracle_port, depth):
    """XF_SUBTREE_MAX_LEVELS = 16: a 17th level leaves the one-launch propagation, and info().fused says so as a fresh build does"""
    h = WE.chains(5, depth, seed=depth)
    n = len(h["parent"])
    par = h["parent"]
    leaves = [e for e in range(n) if e not in set(par.tolist())]
    def second(hs):  # the first edit kept the depth (a one-level world gained its second level)
        info = hs.w.info()
        levels = depth if depth > 1 else 2
        assert (info["n_levels"], info["fused"]) == (levels, 1 if levels <= WE.XF_SUBTREE_MAX_LEVELS else 0), info
        return {"destroy": [leaves[1]], "create": [n]}

    steps = [lambda hs: {"reparent": [(-1, leaves[0])] if depth > 1 else [(1, 0)]}, second, lambda hs: {"reparent": [(leaves[2], n)]}]  # the last one adds a level
    hs = run_script(gpu_ctx, ctx2, oracle_port, h, steps, n_reserve=1, ref_destroy=False)
    info = hs.w.info()
    assert info["n_levels"] == depth + 1
    assert info["fused"] == (1 if depth + 1 <= WE.XF_SUBTREE_MAX_LEVELS else 0)
    assert info["edits"] >= 3


def test_world_heavy_root(gpu_ctx, ctx2, oracle_port):
    """one root whose subtree holds XF_SUBTREE_MAX_RUN + 1 nodes after a re-parent (the per-level launches take over) and fewer again
    after a destroy"""
    fan = WE.XF_SUBTREE_MAX_RUN - 1
    n = 1 + fan + 3  # root 0 with `fan` children = MAX_RUN nodes; 3 more roots
    parent = np.full(n, -1, np.int32)
    parent[1 : 1 + fan] = 0
    rng = np.random.default_rng(3)
    h = {"parent": parent, "local": scenes.random_transforms(rng, n, 30.0)}
    hs = WE.Harness(gpu_ctx, oracle_port, h)
    assert hs.w.info()["fused"] == 1
    hs.edit(reparent=[(0, n - 1)])
    hs.check_oracle("over")
    assert hs.w.info()["fused"] == 0
    hs.check_fresh_build(ctx2, "over")
    hs.edit(destroy=[7, n - 1])
    hs.check_oracle("under")
    assert hs.w.info()["fused"] == 1
    hs.check_fresh_build(ctx2, "under")


def test_world_beyond_the_key_pass_grid(gpu_ctx, oracle_port):
    """more entities than one sweep of the key pass's capped grid (1024 blocks x 256): its second sweep, and the live count of all blocks"""
    h = WE.chains(131100, 2, seed=12)
    n = len(h["parent"])
    assert n > 1024 * 256
    hs = WE.Harness(gpu_ctx, oracle_port, h, n_reserve=2, track=False)
    last_root = int(np.flatnonzero(h["parent"] < 0)[-1])
    kids = np.flatnonzero(h["parent"] >= 0)
    a, b = int(kids[len(kids) // 2]), int(kids[len(kids) // 2 + 1])  # (children of roots in the middle: not under the two destroyed ones)
    hs.edit(destroy=[int(np.flatnonzero(h["parent"] < 0)[0]), last_root], create=[n + 1], reparent=[(n + 1, a), (a, b)])
    hs.check_oracle()
    info = hs.w.info()
    assert (info["n"], info["n_live"]) == (n + 2, int(hs.model.alive.sum()))
    roots = np.flatnonzero(hs.model.alive & (hs.model.parent < 0)).astype(np.int32)
    tr = scenes.random_transforms(hs.rng, len(roots), 2000.0)
    hs.ow.set_transforms(roots, tr)
    hs.w.setTransforms(roots, tr)
    hs.w.propagate()
    hs.check_oracle("after the root moves")


def test_create_cases(gpu_ctx, ctx2, live_oracle):
    """create at n and at n + 70 (growth with holes); destroy and re-create one index in a call; parent under a just-created entity"""
    h = WE.forest(90, seed=11)
    n = 90
    p = h["parent"]
    some_parent = int(p[p >= 0][0])
    steps = [lambda hs: {"create": [n]}, lambda hs: {"create": [n + 70]}, lambda hs: {"create": [n + 5, n + 6], "reparent": [(n + 5, n + 6), (n + 6, 3), (n + 70, n + 5)]}]
    if live_oracle.kind != "reference":
        steps.append(lambda hs: {"destroy": [some_parent], "create": [some_parent], "reparent": [(some_parent, n)]})
    hs = run_script(gpu_ctx, ctx2, live_oracle, h, steps, n_reserve=71, ref_destroy=False)
    assert hs.w.info()["n"] == n + 71
    with pytest.raises(api.LumixError):  # a hole of the growth is dead
        hs.w.setTransforms([n + 30], scenes.random_transforms(np.random.default_rng(0), 1, 1.0))


def test_reparent_cases(gpu_ctx, ctx2, live_oracle):
    """across trees, to a deeper and a shallower level, detach, siblings arriving in descending entity order, A under B then B under C"""
    h = WE.chains(12, 4, seed=9)
    par = h["parent"]
    n = len(par)
    m = WE.Model(par)
    d = m.depth()
    roots = [int(e) for e in np.flatnonzero(par < 0)]
    by_depth = {k: [int(e) for e in np.flatnonzero(d == k)] for k in range(4)}
    a, b, c = by_depth[1][0], roots[3], by_depth[2][5]
    steps = [
        lambda hs: {"reparent": [(roots[1], by_depth[3][0])]},               # across trees, to a shallower level
        lambda hs: {"reparent": [(by_depth[3][2], by_depth[1][4])]},         # ... to a deeper level, with its subtree
        lambda hs: {"reparent": [(-1, by_depth[2][7])]},                      # detach
        lambda hs: {"reparent": [(roots[2], e) for e in sorted(roots[6:10], reverse=True)]},  # siblings in descending entity order
        lambda hs: {"reparent": [(b, a), (c, b)]},                            # A under B, then B under C
        lambda hs: {"reparent": [(roots[5], a), (roots[4], a)]},              # one child twice: the last parent holds
    ]
    run_script(gpu_ctx, ctx2, live_oracle, h, steps)


def test_destroy_subtree_with_listed_descendant(gpu_ctx, ctx2, live_oracle):
    h = WE.chains(10, 4, seed=2)
    par = h["parent"]
    m = WE.Model(par)
    root = int(np.flatnonzero(par < 0)[2])
    sub = m.subtree(root)
    steps = [lambda hs: {"destroy": [root, sub[-1]]}, lambda hs: {"destroy": [sub2 for sub2 in m.subtree(int(np.flatnonzero(par < 0)[4]))[1:2]]}]
    hs = run_script(gpu_ctx, ctx2, live_oracle, h, steps)
    assert hs.w.info()["n_live"] == len(par) - len(sub) - 3


def test_cycle_in_the_middle_is_refused(gpu_ctx, oracle_port):
    """refused, and nothing changed: getTransforms / getLocalTransforms are bit-identical to before, so is the next propagation"""
    h = WE.chains(8, 4, seed=4)
    hs = WE.Harness(gpu_ctx, oracle_port, h)
    par = h["parent"]
    d = WE.Model(par).depth()
    leaf = int(np.flatnonzero(d == 3)[0])
    top = leaf
    while par[top] >= 0:
        top = int(par[top])
    other = int(np.flatnonzero(par < 0)[5])
    before = (hs.w.getTransforms().tobytes(), hs.w.getLocalTransforms().tobytes(), hs.w.info())
    with pytest.raises(api.LumixError):
        hs.w.edit(destroy=[int(np.flatnonzero(par < 0)[6])], create=[len(par)], create_transforms=scenes.random_transforms(hs.rng, 1, 5.0),
                  reparent=[(other, leaf), (leaf, top), (top, other)])  # the third closes other -> leaf -> top -> other
    assert (hs.w.getTransforms().tobytes(), hs.w.getLocalTransforms().tobytes(), hs.w.info()) == before
    hs.write()
    hs.w.propagate()
    hs.check_oracle("after the refused batch")
    hs.edit(reparent=[(other, leaf), (leaf, top)])  # the same batch without the closing entry is fine
    hs.check_oracle("after the accepted batch")


def test_error_cases_leave_the_edit_count(gpu_ctx, oracle_port):
    h = WE.chains(6, 3, seed=6)
    hs = WE.Harness(gpu_ctx, oracle_port, h)
    n = len(h["parent"])
    root = int(np.flatnonzero(h["parent"] < 0)[1])
    dead = hs.edit(destroy=[root])
    assert len(dead) == 3
    edits = hs.w.info()["edits"]
    one = scenes.random_transforms(hs.rng, 1, 5.0)
    before = hs.snapshot()
    with pytest.raises(api.LumixError):
        hs.w.setTransforms([dead[1]], one)  # a staging call on a dead entity
    with pytest.raises(api.LumixError):
        hs.w.setWorldTransforms([dead[2]], one)
    with pytest.raises(api.LumixError):
        hs.w.edit(reparent=[(0 if dead[0] != 0 else 3, dead[2])])  # a dead child
    with pytest.raises(api.LumixError):
        hs.w.edit(reparent=[(n, 0)])  # an out-of-range parent
    with pytest.raises(api.LumixError):
        hs.w.edit(create=[n, n], create_transforms=np.concatenate([one, one]))  # a duplicate create
    with pytest.raises(api.LumixError):
        hs.w.edit(create=[0 if dead[0] != 0 else 3], create_transforms=one)  # a live index
    with pytest.raises(api.LumixError):
        hs.w.edit(destroy=[dead[0]])
    assert hs.w.info()["edits"] == edits and hs.w.info()["n"] == n
    assert hs.snapshot() == before
    hs.w.propagate()
    hs.check_oracle()


def test_pending_writes_are_propagated_first(gpu_ctx, oracle_port):
    """a write staged and not propagated: the edit's implied propagation shows in the moved list, and the result is the oracle's eager order"""
    h = WE.chains(20, 3, seed=8)
    hs = WE.Harness(gpu_ctx, oracle_port, h)
    par = h["parent"]
    hs.w.readMoved()
    roots = np.flatnonzero(par < 0).astype(np.int32)
    kid = int(np.flatnonzero(par == roots[3])[0])
    tr = scenes.random_transforms(hs.rng, 2, 500.0)
    moved_roots = roots[[3, 7]]
    hs.ow.set_transforms(moved_roots, tr)
    hs.w.setTransforms(moved_roots, tr)  # staged, not propagated
    hs.edit(reparent=[(int(roots[5]), kid)])  # setParent reads kid's NEW world transform in the oracle
    hs.check_oracle("edit with a pending write")
    ent, _ = hs.w.readMoved()
    want = set(hs.model.subtree(int(roots[7]))) | set(WE.Model(par).subtree(int(roots[3])))
    assert set(ent.tolist()) == want
    hs.edit(reparent=[(-1, kid)])  # nothing staged: no propagation, nothing moved
    assert len(hs.w.readMoved()[0]) == 0
    hs.check_oracle()


def test_destroy_bound_entity_keeps_the_other_spheres_moving(gpu_ctx, live_oracle):
    """culling bindings survive an edit; a destroyed entity's is dropped (its sphere stays where it was). Through a cull, as
    test_world_moves_refresh_culling does."""
    h = scenes.hierarchy_chains(300, 3, seed=4, root_extent=1500.0)
    n = len(h["parent"])
    hs = WE.Harness(gpu_ctx, live_oracle, h, ref_destroy=False, track=False)
    rng = np.random.default_rng(33)
    model_radius = rng.uniform(0.5, 40.0, n).astype(np.float32)
    ocs = live_oracle.culling_system()
    tr0 = hs.ow.get_transforms()[:n]
    ent = np.arange(n, dtype=np.int32)
    r0 = model_radius * tr0["scale"].max(axis=1)
    ocs.add_bulk(ent, np.zeros(n, np.uint8), tr0["pos"], r0)
    hs.ow.bind_culling(ocs, ent, model_radius)
    cs = api.CullingSystem(gpu_ctx)
    cs.build(ent, np.zeros(n, np.uint8), tr0["pos"], r0)
    hs.w.bindCulling(ent, model_radius)
    fr = np.concatenate([api.viewport_frustum(pos=(0, 0, 2000.0)), api.viewport_frustum(pos=(300.0, 50.0, -100.0), rot=H.quat_from_yaw_pitch(1.0, 0.1))])
    roots = np.flatnonzero(h["parent"] < 0).astype(np.int32)

    def frame(what):
        live_roots = np.array([r for r in roots if hs.model.alive[r] and hs.model.parent[r] < 0], np.int32)
        new_root = hs.ow.get_transforms()[live_roots]
        new_root["pos"] += rng.uniform(-300.0, 300.0, size=(len(live_roots), 3))
        hs.ow.set_transforms(live_roots, new_root)
        hs.w.setTransforms(live_roots, new_root)
        hs.w.propagate()
        hs.check_oracle(what)
        res = cs.cull(fr)
        for f in range(len(fr)):
            ids, types, _ = ocs.cull(fr[f : f + 1])
            got_ids, got_types = res.all_ids(f)
            H.assert_same_visible(H.sorted_by_type(got_ids, got_types), H.sorted_by_type(ids, types), f"{what} frustum {f}")

    for fused in (1, 0):
        hs.w.setOption(api.WORLD_OPT_FUSED_LEVELS, fused)
        frame(f"before (fused {fused})")
        kid = int(np.flatnonzero(h["parent"] == roots[10 + fused])[0])
        hs.edit(destroy=[int(roots[3 + fused])], reparent=[(int(roots[20 + fused]), int(roots[1 + fused])), (-1, kid)])
        frame(f"after the edit (fused {fused})")
        frame(f"a second frame (fused {fused})")
    hs.w.setOption(api.WORLD_OPT_FUSED_LEVELS, 1)


def test_destroyed_binding_stays_dropped_when_the_index_returns(gpu_ctx, oracle_port):
    """The engine's free list hands a destroyed index straight back. The binding of the entity that died must not come back with the
    index - not when the binding tables are stated again from the host's list (after lmx_world_set_parent, after the culling set was
    laid out again) - and an entity the engine already took out of the culling system must not fail the edit's own propagation."""
    h = scenes.hierarchy_chains(100, 3, seed=7, root_extent=800.0)
    par = h["parent"]
    n = len(par)
    hs = WE.Harness(gpu_ctx, oracle_port, h, ref_destroy=False, track=False)
    rng = np.random.default_rng(9)
    model_radius = rng.uniform(0.5, 40.0, n).astype(np.float32)
    tr0 = hs.ow.get_transforms()[:n]
    ent = np.arange(n, dtype=np.int32)
    cs = api.CullingSystem(gpu_ctx)
    cs.build(ent, np.zeros(n, np.uint8), tr0["pos"], model_radius * tr0["scale"].max(axis=1))
    hs.w.bindCulling(ent, model_radius)
    hs.w.propagate()
    roots = np.flatnonzero(par < 0).astype(np.int32)
    d = WE.Model(par).depth()
    leaves = np.flatnonzero(d == 2).astype(np.int32)
    back, gone, other = int(leaves[3]), int(leaves[8]), int(roots[20])

    def scaled(e, k):
        t = hs.w.getTransforms()[e : e + 1].copy()
        t["scale"] = np.float32(k)
        t["pos"] += 3.0
        return t

    def move_root(e, k, what):  # a bound, live root follows its transform
        hs.w.setTransforms([e], scaled(e, k))
        hs.w.propagate()
        assert cs.getRadius(e) == float(model_radius[e] * np.float32(k)), what

    radius_before = cs.getRadius(back)
    # 1. destroyed and created again in one call; then every way the tables are stated again
    hs.edit(destroy=[back], create=[back])
    for k, again in ((2.0, lambda: None), (3.0, lambda: hs.w.setParent(int(roots[1]), int(roots[2]))), (4.0, lambda: cs.compact())):
        again()
        hs.w.setTransforms([back], scaled(back, k))  # the new entity of that index is a root: its world transform, its scale
        hs.w.propagate()
        assert cs.getRadius(back) == radius_before, f"the dropped binding came back (scale {k})"
        move_root(other, k, f"a surviving binding stopped following (scale {k})")
    # 2. the engine removed the entity from the culling system first, a write is pending, and the binding tables are unstated
    hs.model.parent[int(roots[2])] = int(roots[1])  # (the set_parent above, for the model's depth order)
    cs.remove(gone)
    hs.w.setParent(-1, int(roots[2]))
    hs.w.setTransforms([other], scaled(other, 5.0))
    hs.w.edit(destroy=[gone])
    assert cs.getRadius(other) == float(model_radius[other] * np.float32(5.0))
    cs.compact()
    move_root(other, 6.0, "after the culling set was laid out again")
    assert hs.w.info()["n_live"] == n - 1


@pytest.mark.parametrize("removed_first", [True, False], ids=["removed-from-culling", "index-returns"])
def test_binding_voided_by_the_edits_own_propagation_stays_dropped(gpu_ctx, oracle_port, removed_first):
    """The edit's own propagation states the binding tables again (a write is pending and lmx_world_bind_culling left them unstated) and
    leaves the entry of the entity the batch kills void. The host's list must void it too: when the dynamic culling set is laid out
    again afterwards (an overflow reserve bumps its generation) and the tables are stated a third time, the propagation must not fail
    on an entity the engine had removed from the culling system, and the binding must not come back for a new entity of that index."""
    h = scenes.hierarchy_chains(100, 3, seed=7, root_extent=800.0)
    par = h["parent"]
    n = len(par)
    hs = WE.Harness(gpu_ctx, oracle_port, h, ref_destroy=False, track=False)
    rng = np.random.default_rng(10)
    model_radius = rng.uniform(0.5, 40.0, n).astype(np.float32)
    tr0 = hs.ow.get_transforms()[:n]
    ent = np.arange(n, dtype=np.int32)
    cs = api.CullingSystem(gpu_ctx)
    cs.build(ent, np.zeros(n, np.uint8), tr0["pos"], model_radius * tr0["scale"].max(axis=1))
    hs.w.bindCulling(ent, model_radius)  # the tables are unstated from here
    roots = np.flatnonzero(par < 0).astype(np.int32)
    leaves = np.flatnonzero(WE.Model(par).depth() == 2).astype(np.int32)
    gone, other = int(leaves[8]), int(roots[20])

    def scaled(e, k):
        t = tr0[e : e + 1].copy()
        t["scale"] = np.float32(k)
        t["pos"] += 3.0 * k
        return t

    radius_before = cs.getRadius(gone)
    if removed_first:
        cs.remove(gone)
    hs.w.setTransforms([other], scaled(other, 2.0))  # staged: the edit propagates first, and that propagation states the tables
    hs.w.edit(destroy=[gone])
    assert cs.getRadius(other) == float(model_radius[other] * np.float32(2.0))
    if not removed_first:
        hs.w.edit(create=[gone], create_transforms=scaled(gone, 1.0))
    cs.setOption(api.CULL_OPT_OVERFLOW_RESERVE, 64)  # the dynamic set is laid out again: every table is stated from the host's list
    if not removed_first:
        hs.w.setTransforms([gone], scaled(gone, 7.0))
    hs.w.setTransforms([other], scaled(other, 3.0))
    hs.w.propagate()
    assert cs.getRadius(other) == float(model_radius[other] * np.float32(3.0)), "a surviving binding stopped following"
    if not removed_first:
        assert cs.getRadius(gone) == radius_before, "the dropped binding came back with the index"
    hs.w.setTransforms([other], scaled(other, 4.0))
    hs.w.propagate()  # and every later propagation
    assert cs.getRadius(other) == float(model_radius[other] * np.float32(4.0))
    assert hs.w.info()["n_live"] == (n - 1 if removed_first else n)


def test_destroy_attached_entity_and_attachment_parent(gpu_ctx, oracle_port):
    """bone attachments survive an edit that renumbers the slots; those of a destroyed entity, or whose parent entity was destroyed, are
    dropped: the remaining attached entities still follow their bones after lmx_skin_run (golden of test_bone_attachments_golden_and_subtrees)"""
    g, ga = np.load(os.path.join(G, "skin.npz")), np.load(os.path.join(G, "attach.npz"))
    sk = api.Skinning(gpu_ctx)
    sk.setMode(True)
    model = sk.addModel(g["parents"], g["bind"], int(g["first_nonroot"][0]))
    mesh = sk.addMesh(g["verts"], g["skin"])
    n_inst = g["rel_pos"].shape[0]
    sk.setInstances([model] * n_inst, [mesh] * n_inst)
    sk.uploadPoses(g["rel_pos"], g["rel_rot"])
    n = len(ga["parent"])
    rng = np.random.default_rng(23)
    tr = np.zeros(3 * n, api.TRANSFORM)
    tr[:n] = ga["parent"]
    tr[n : 2 * n] = scenes.random_transforms(rng, n, 100.0)
    tr["scale"][n : 2 * n] = ga["scale"]
    tr[2 * n :] = scenes.random_transforms(rng, n, 3.0)
    parent = np.full(3 * n, -1, np.int32)
    parent[2 * n :] = np.arange(n, 2 * n)
    w = api.World(gpu_ctx)
    w.build(parent, tr)
    w.setBoneAttachments(np.arange(n, 2 * n), np.arange(n), ga["instance"], ga["bone"], ga["relative"])
    sk.run()
    w.updateBoneAttachments()
    w.propagate()
    assert H.transforms_bits_equal(w.getTransforms()[n : 2 * n], ga["result"])
    # destroy attached entity n + 3 (its child goes along) and the parent entity 5 of attachment n + 5; detach a child and hang a parent
    # entity under another: every slot is renumbered
    w.edit(destroy=[n + 3, 5], reparent=[(-1, 2 * n + 7), (0, 1)])
    assert w.info()["n_live"] == 3 * n - 3
    moved = tr[n : 2 * n].copy()
    moved["pos"] += 5.0
    alive = np.ones(n, bool)
    alive[3] = False
    w.setTransforms(np.arange(n, 2 * n)[alive], moved[alive])
    w.propagate()
    w.updateBoneAttachments()
    w.propagate()
    got = w.getTransforms()
    follows = alive.copy()
    follows[5] = False
    assert H.transforms_bits_equal(got[n : 2 * n][follows], ga["result"][follows])
    assert H.transforms_bits_equal(got[n + 5 : n + 6], moved[5:6]), "the attachment of a destroyed parent entity still ran"
    kids = follows.copy()
    kids[7] = False  # detached
    assert H.transforms_bits_equal(got[2 * n :][kids], oracle_port.compose(ga["result"], tr[2 * n :])[kids])
    sk.setMode(False)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_world_edit_fuzz(gpu_ctx, ctx2, live_oracle, seed):
    """200 steps on a 300-entity world: a batch of up to 8 edits of each kind, then random root and child writes and a propagate;
    (a) every step, (b) every 20th"""
    h = WE.forest(300, seed=40 + seed)
    n_total = 340
    recreate = live_oracle.kind != "reference"
    hs = WE.Harness(gpu_ctx, live_oracle, h, n_reserve=n_total - 300, ref_destroy=not recreate)
    rng = np.random.default_rng(seed)
    ever = np.zeros(n_total, bool)
    refused = 0
    for i in range(200):
        ever[: hs.model.n] |= hs.model.alive
        d, c, r = WE.random_batch(rng, hs.model, n_total, recreate=recreate, ever_created=ever)
        if i % 25 == 7 and len(r) >= 1:  # a batch that closes a cycle with its last entry: refused whole
            p, ch = r[-1]
            if p >= 0:
                bad = r + [(ch, p)]
                edits = hs.w.info()["edits"]
                with pytest.raises(api.LumixError):
                    hs.w.edit(destroy=d, create=c, create_transforms=scenes.random_transforms(rng, len(c), 9.0), reparent=bad)
                assert hs.w.info()["edits"] == edits
                refused += 1
        killed = hs.edit(destroy=d, create=c, reparent=r)
        hs.check_oracle(f"seed {seed} step {i}")
        ent, _ = hs.w.readMoved()  # what the last propagation - the previous step's, or the one inside this edit - moved
        assert np.isin(ent, np.concatenate([hs.model.live(), np.array(killed, np.int32)])).all(), "an entity that was dead at the propagation is in the moved list"
        hs.write(frac=0.1)
        if i % 3:
            hs.w.propagate()
            hs.check_oracle(f"seed {seed} step {i} after the writes")  # (else: the next edit propagates)
        if i % 20 == 19:
            hs.w.propagate()
            hs.check_fresh_build(ctx2, f"seed {seed} step {i}")
    assert hs.w.info()["edits"] == 200
