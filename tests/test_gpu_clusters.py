"""fillClusters on the device (lmx_clusters_*, cluster_kernels.hip) against tests/cluster_oracle.py: light and probe records, `clusters` and
`map` byte for byte - hand-made lights on a 2 x 1 x 16 grid, the probes' order and the segments' order, ~3000 seeded lights on a 1920 x 1080
view with lights placed on the wave, tile and block edges of the list, the chain cull -> clusters with the list's length on the device only,
overflow of either buffer, and the errors. Then the recorded reference fixture (tests/golden/clusters_small.npz) and the kernels' edges: probe
counts past a wave step, a tile and at the most of a kind, the grids 64 x 64 x 16, 64 x 1, 1 x 64 and an orthographic view, a list beyond
one sweep of the record step, the saturating prefix, a map capacity in the middle of the grid, a short run behind a long one, and
transforms read from the world hierarchy across a World.edit. The oracle itself is held to the reference by
tests/test_cluster_oracle_vs_ref.py."""
import numpy as np
import pytest

from lumixengine_amd import api
from tests import cluster_oracle as CO

pytestmark = pytest.mark.gpu

CAM = np.array(CO.CAM_POS)
BIG = 1 << 22  # a map capacity no case here reaches


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own: the tables and the transform source of the draw pass stay out of the other modules' way."""
    c = api.Context(0)
    yield c
    c.close()


def filler(ctx, transforms, lights, atlas=None, probes=None, max_lights=4096, map_capacity=BIG):
    dc = api.DrawCommands(ctx)
    dc.bindWorld(False)
    dc.setTransforms(transforms)
    cf = api.ClusterFiller(ctx)
    cf.setLights(lights)
    cf.setAtlas(atlas)
    cf.setProbes(**(probes or {}))
    cf.reserve(max_lights, map_capacity)
    return cf


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if got.tobytes() != want.tobytes():
        g, w = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first at {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}")


def assert_run_matches(cf, want, what=""):
    cnt = cf.counts()
    assert cnt == {"lights": len(want["lights"]), "env_probes": len(want["env_probes"]), "refl_probes": len(want["refl_probes"]), "map_entries": len(want["map"]),
                   "overflow": 0}, what
    clusters, size = cf.readClusters()
    assert size == want["size"], what
    same_bytes(cf.readLights(), want["lights"], what + " lights")
    same_bytes(clusters, want["clusters"], what + " clusters")
    same_bytes(cf.readMap(), want["map"], what + " map")
    env, refl = cf.readProbes()
    same_bytes(env, want["env_probes"], what + " env probes")
    same_bytes(refl, want["refl_probes"], what + " refl probes")


def segments(want, c):
    cl = want["clusters"][c]
    o, nl, ne, nr = (int(cl[k]) for k in ("offset", "lights_count", "env_probes_count", "refl_probes_count"))
    m = want["map"]
    return m[o : o + nl].tolist(), m[o + nl : o + nl + ne].tolist(), m[o + nl + ne : o + nl + ne + nr].tolist()


def clusters_of(want, light):
    return [c for c in range(len(want["clusters"])) if light in segments(want, c)[0]]


# ---- hand-made lights on 128 x 64 (2 x 1 x 16 clusters) ---------------------------------------------------------------------------
def test_hand_made_lights(ctx):
    view, names, tr, lights, radius = CO.hand_made()
    n = len(names)
    listed = np.arange(n, dtype=np.int32)
    want = CO.fill_clusters(view, listed, tr, lights)
    rg = {k: want["ranges"][i].tolist() for i, k in enumerate(names)}
    # what the cases are about, on the oracle's side
    assert len(clusters_of(want, names.index("inside"))) == 1
    assert rg["straddles_x"][0] == [0, 2] and len(clusters_of(want, names.index("straddles_x"))) == 2
    for k, axis in (("left", 0), ("right", 0), ("above", 1), ("below", 1), ("before_near", 2), ("beyond_far", 2)):
        assert rg[k][axis] == [-1, -1] and not clusters_of(want, names.index(k)), k
    assert np.float32(radius["left"]) > 0 and {tuple(rg["left"][0]), tuple(rg["right"][0])} == {(-1, -1)}
    assert rg["dist_eq_r"][2][0] == 2 and rg["dist_gt_r"][2][0] == 3
    assert rg["dist_eq_minus_r"][2][1] == 5 and rg["dist_lt_minus_r"][2][1] == 4
    assert rg["nan"] == [[0, 2], [0, 1], [0, 16]]  # a NaN distance fails `<` and `>` alike: every cluster
    assert len(clusters_of(want, names.index("radius_0"))) == 1
    assert len(clusters_of(want, names.index("everything"))) == 32
    assert not clusters_of(want, names.index("past_tables")) and not want["lights"][n - 1]["radius"]
    cf = filler(ctx, tr, lights)
    cf.runList(view, listed)
    assert_run_matches(cf, want, "hand-made")
    got = cf.readLights()
    assert not got["padding"].view(np.uint32).any() and (got["atlas_idx"] == 0xFFFFFFFF).all()
    assert cf.readLightEntities().tolist() == listed.tolist()


# ---- records ----------------------------------------------------------------------------------------------------------------------
def test_records_byte_for_byte(ctx):
    sc = CO.scene()
    view = CO.view(128, 64)  # fp64 camera at (1e6, 50, -1e6): Vec3(light_pos - cam_pos) is one rounding of an fp64 difference
    listed = np.random.default_rng(8).choice(CO.N_ENTITIES + 40, 200, replace=False).astype(np.int32)  # some past the tables
    assert (listed >= CO.N_ENTITIES).any()
    short_atlas = sc["atlas"][:3000]  # a table that does not cover every listed entity: those read 0
    assert ((listed >= 3000) & (listed < CO.N_ENTITIES)).any()
    for atlas, what in ((None, "no atlas table"), (short_atlas, "atlas table")):
        cf = filler(ctx, sc["transforms"], sc["lights"], atlas)
        cf.runList(view, listed)
        want = CO.light_records(listed, sc["transforms"], sc["lights"], atlas, CAM)
        got = cf.readLights()
        same_bytes(got, want, what)
        assert not got["padding"].view(np.uint32).any(), "the 8 padding bytes are zero"
        assert cf.readLightEntities().tolist() == listed.tolist()
        if atlas is None:
            assert (got["atlas_idx"] == 0xFFFFFFFF).all()
        else:
            assert set(got["atlas_idx"].tolist()) > {0xFFFFFFFF, 0}
    # the record's position is the fp64 difference rounded once - not a difference of rounded values
    i = int(np.flatnonzero(listed < CO.N_ENTITIES)[0])
    assert got["pos"][i].tolist() == (sc["transforms"]["pos"][listed[i]] - CAM).astype(np.float32).tolist()
    assert got["pos"][i].tolist() != (sc["transforms"]["pos"][listed[i]].astype(np.float32) - CAM.astype(np.float32)).tolist()


# ---- probes -----------------------------------------------------------------------------------------------------------------------
def test_probes_order_and_segments(ctx):
    sc = CO.scene()
    view = CO.view(128, 64)
    probes = {k: sc[k] for k in ("env", "env_entities", "refl", "refl_entities")}
    listed = np.arange(0, 600, dtype=np.int32)
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes)
    cf.runList(view, listed)
    want = CO.fill_clusters(view, listed, sc["transforms"], sc["lights"], sc["atlas"], **probes)
    assert_run_matches(cf, want, "probes")
    env, refl = cf.readProbes()
    # disabled probes are left out; equal volumes keep module order (probes 1 and 4 of the scene's environment probes, 0 and 5 of its reflection probes)
    assert len(env) == 7 and len(refl) == 6
    order = CO._probe_order(sc["env"]["flags"], sc["env"]["outer_range"]).tolist()  # module indices in output order
    assert order.index(4) == order.index(1) + 1
    vol = env["outer_range"][:, 0] * env["outer_range"][:, 1] * env["outer_range"][:, 2]
    assert (np.diff(vol) >= 0).all() and (np.diff(vol) == 0).any()
    tie = int(np.flatnonzero(np.diff(vol) == 0)[0])
    ents = sc["env_entities"]
    tr = sc["transforms"]
    assert env["pos"][tie].tolist() == (tr["pos"][ents[1]] - CAM).astype(np.float32).tolist() and env["pos"][tie + 1].tolist() == (tr["pos"][ents[4]] - CAM).astype(np.float32).tolist()
    assert 2 not in order and 7 not in order
    assert (env["rot"][:, 3] == -tr["rot"][ents[order], 3]).all() and (env["rot"][:, :3] == tr["rot"][ents[order], :3]).all()  # conjugated: w negated
    # some cluster holds all three kinds: its segment is lights, then environment probes, then reflection probes, each ascending
    cl = want["clusters"]
    full = np.flatnonzero((cl["lights_count"] > 1) & (cl["env_probes_count"] > 1) & (cl["refl_probes_count"] > 1))
    assert len(full)
    got_map = cf.readMap()
    for c in full[:4]:
        o, nl, ne, nr = (int(cl[c][k]) for k in ("offset", "lights_count", "env_probes_count", "refl_probes_count"))
        seg = got_map[o : o + nl + ne + nr]
        for part in (seg[:nl], seg[nl : nl + ne], seg[nl + ne :]):
            assert (np.diff(part) > 0).all()
        assert seg[nl : nl + ne].max() < len(env) and seg[nl + ne :].max() < len(refl)


# ---- ~3000 seeded lights on 1920 x 1080 -------------------------------------------------------------------------------------------
N_SEEDED = CO.N_SEEDED
seeded_case = CO.seeded_case  # (view, listed, probes, want), computed once


def test_seeded_lights_1920x1080(ctx):
    sc = CO.scene()
    view, listed, probes, want = seeded_case()
    assert want["size"] == (30, 17, 16) and N_SEEDED > 4 * api.CLUSTER_BLOCK * 2  # several waves, tiles and blocks of every kernel
    counts = want["clusters"]["lights_count"]
    assert counts.min() >= 1 and counts.max() > 64 and len(want["map"]) > 100000  # some cluster's segment spans more than one wave step
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes)
    cf.runList(view, listed)
    assert_run_matches(cf, want, "seeded")
    first = (cf.readLights().tobytes(), cf.readClusters()[0].tobytes(), cf.readMap().tobytes())
    cf.runList(view, listed)
    assert (cf.readLights().tobytes(), cf.readClusters()[0].tobytes(), cf.readMap().tobytes()) == first, "two runs give identical bytes"


# ---- cull -> clusters -------------------------------------------------------------------------------------------------------------
def test_chain_cull_to_clusters(ctx):
    sc = CO.scene()
    n = 1500
    rng = np.random.default_rng(12)
    ents = np.arange(n, dtype=np.int32)
    types = np.where(rng.random(n) < 0.5, 2, 0).astype(np.uint8)  # LOCAL_LIGHT and MESH
    cs = api.CullingSystem(ctx)
    cs.build(ents, types, sc["transforms"]["pos"][:n], np.maximum(sc["lights"]["range"][:n], 0.01))
    view = CO.view(1920, 1080)
    probes = {k: sc[k] for k in ("env", "env_entities", "refl", "refl_entities")}
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes)
    res = cs.cull(view["frustum"], api.TYPE_ALL, view=3)
    cf.run(view, cull_view=3)  # nothing between the cull and the run reads a count back
    listed = cf.readLightEntities()
    visible = res.ids(0, 2)
    assert 20 < len(visible) < (types == 2).sum() and sorted(listed.tolist()) == sorted(visible.tolist())
    assert (types[listed] == 2).all()
    want = CO.fill_clusters(view, listed, sc["transforms"], sc["lights"], sc["atlas"], **probes)
    assert_run_matches(cf, want, "chain")
    # a cull of the LOCAL_LIGHT type alone serves too; one of another type does not
    cs.cull(view["frustum"], 2, view=3)
    cf.run(view, cull_view=3)
    assert sorted(cf.readLightEntities().tolist()) == sorted(visible.tolist())
    cs.cull(view["frustum"], 0, view=3)
    with pytest.raises(api.LumixError) as e:
        cf.run(view, cull_view=3)
    assert e.value.code == 6  # LMX_ERR_NOT_BUILT


# ---- overflow ---------------------------------------------------------------------------------------------------------------------
def test_overflow_reports_the_needed_sizes_and_writes_nothing_past_a_buffer(ctx):
    sc = CO.scene()
    view, listed, probes, want = seeded_case()
    n, need = len(listed), len(want["map"])
    guard_records, guard_words = api.CLUSTERS_GUARD_BYTES // 64, api.CLUSTERS_GUARD_BYTES // 4

    def guards_intact(cf):
        assert (cf.readLights(cf.max_lights + guard_records)[cf.max_lights :].view(np.uint8) == 0xA5).all(), "light records"
        assert (cf.readLightEntities(cf.max_lights + guard_words)[cf.max_lights :].view(np.uint8) == 0xA5).all(), "light entities"
        assert (cf.readMap(cf.map_capacity + guard_words)[cf.map_capacity :].view(np.uint8) == 0xA5).all(), "map"

    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes, max_lights=n - 1, map_capacity=need)
    cf.runList(view, listed)
    cnt = cf.counts()
    assert cnt["overflow"] == 1 and cnt["lights"] == n and cnt["map_entries"] == need, cnt
    guards_intact(cf)
    cf.reserve(n, need - 1)
    cf.runList(view, listed)
    cnt = cf.counts()
    assert cnt["overflow"] == 2 and cnt["lights"] == n and cnt["map_entries"] == need, cnt
    guards_intact(cf)
    cf.reserve(n - 1, need - 1)
    cf.runList(view, listed)
    assert cf.counts()["overflow"] == 3
    guards_intact(cf)
    cf.reserve(n, need)  # exactly what the counts asked for
    cf.runList(view, listed)
    assert_run_matches(cf, want, "after the larger reserve")
    guards_intact(cf)
    with pytest.raises(api.LumixError) as e:
        cf.readMap(need - 1)
    assert e.value.code == 5


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors():
    fresh = api.Context(0)
    try:
        cf = api.ClusterFiller(fresh)
        view = CO.view(128, 64)
        with pytest.raises(api.LumixError) as e:
            cf.runList(view, np.zeros(1, np.int32))
        assert e.value.code == 6  # no tables
        cf.setLights(np.zeros(4, api.POINT_LIGHT))
        with pytest.raises(api.LumixError) as e:
            cf.runList(view, np.zeros(1, np.int32))
        assert e.value.code == 6  # no reserve
        cf.reserve(16, 1024)
        with pytest.raises(api.LumixError) as e:
            cf.run(view, cull_view=0)
        assert e.value.code == 6  # the slot holds no cull result
        with pytest.raises(api.LumixError) as e:
            cf.counts()
        assert e.value.code == 6  # nothing has run
        with pytest.raises(api.LumixError) as e:
            cf.setProbes(env=np.zeros(api.CLUSTER_MAX_PROBES + 1, api.ENV_PROBE), env_entities=np.zeros(api.CLUSTER_MAX_PROBES + 1, np.int32))
        assert e.value.code == 5  # LMX_ERR_CAPACITY
        with pytest.raises(api.LumixError) as e:
            cf.setProbes(refl=np.zeros(api.CLUSTER_MAX_PROBES + 1, api.REFL_PROBE), refl_entities=np.zeros(api.CLUSTER_MAX_PROBES + 1, np.int32))
        assert e.value.code == 5
        with pytest.raises(api.LumixError) as e:
            cf.runList(CO.view(4097, 64), np.zeros(1, np.int32))
        assert e.value.code == 5
        cf.setProbes(env=np.zeros(api.CLUSTER_MAX_PROBES, api.ENV_PROBE), env_entities=np.zeros(api.CLUSTER_MAX_PROBES, np.int32))  # 1024 of a kind are fine (all disabled)
        cf.runList(view, np.zeros(0, np.int32))  # an empty list: every cluster empty
        assert cf.counts() == {"lights": 0, "env_probes": 0, "refl_probes": 0, "map_entries": 0, "overflow": 0}
        clusters, size = cf.readClusters()
        assert size == (2, 1, 16) and not clusters.view(np.uint32).any()
    finally:
        fresh.close()


# ---- the recorded reference -------------------------------------------------------------------------------------------------------
def test_golden_fixture(ctx):
    """tests/golden/clusters_small.npz - the reference's own output, recorded by tests/golden/make_golden_clusters.py - byte for byte."""
    sc, listed, probes, views = CO.golden_small()
    cf = filler(ctx, sc["transforms"], sc["lights"], None, probes)
    for view, want in views:
        assert len(want["map"]) > 500 and len(want["lights"]) == len(listed) and len(want["env_probes"]) == len(want["refl_probes"]) == 12
        cf.runList(view, listed)
        assert_run_matches(cf, want, f"fixture {want['size']}")


# ---- probe counts on the wave, tile and table edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_env,n_refl", [(63, 65), (64, 64), (255, 257), (256, 1), (1024, 1024)])
def test_probe_counts_past_a_wave_and_a_tile(ctx, n_env, n_refl):
    """The two probe walks of the gather past one wave step (64), one tile (CLUSTER_BLOCK) and at the most of a kind, the reflection walk's
    base behind n_env entries, the record step's probe blocks up to all of their threads. ENABLED counts land on the edges: a few
    disabled probes are mixed in wherever the tables (at most CLUSTER_MAX_PROBES of a kind) have room for them."""
    sc = CO.scene()
    view = CO.view(128, 64)
    edges = (0, 63, 64, api.CLUSTER_BLOCK - 1, api.CLUSTER_BLOCK, n_env - 1, n_refl - 1)
    disabled = min(3, api.CLUSTER_MAX_PROBES - max(n_env, n_refl))
    assert (disabled == 0) == (n_env == api.CLUSTER_MAX_PROBES)
    probes = CO.probe_tables(n_env, n_refl, seed=40 + n_env, disabled=disabled, wide=edges, far=0.1 if max(n_env, n_refl) > 200 else 0.0)
    assert len(probes["env"]) == n_env + disabled and len(probes["refl"]) == n_refl + disabled
    listed = np.arange(100, dtype=np.int32)
    want = CO.fill_clusters(view, listed, sc["transforms"], sc["lights"], sc["atlas"], **probes)
    assert (len(want["env_probes"]), len(want["refl_probes"])) == (n_env, n_refl)
    cl = want["clusters"]
    both = np.ones(len(cl), bool)
    for n, field in ((n_env, "env_probes_count"), (n_refl, "refl_probes_count")):
        if n > 64:  # more than one wave step
            both &= cl[field] > 64
        if n == api.CLUSTER_MAX_PROBES:  # more than one tile
            both &= cl[field] > api.CLUSTER_BLOCK
        if n <= 64:
            both &= cl[field] == n  # every probe of the kind: a full (or all but full) wave step
    assert both.any(), "no cluster whose two probe segments pass the steps this case is about"
    c = int(np.flatnonzero(both)[0])
    _, env_seg, refl_seg = segments(want, c)
    for n, seg in ((n_env, env_seg), (n_refl, refl_seg)):
        assert {e for e in edges if 0 <= e < n} <= set(seg)  # the scene-wide probes on the edge indices
    assert min(len(segments(want, k)[1]) for k in range(len(cl))) >= len({e for e in edges if 0 <= e < n_env})
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes)
    cf.runList(view, listed)
    assert_run_matches(cf, want, f"probes {n_env} + {n_refl}")


# ---- grid shapes ------------------------------------------------------------------------------------------------------------------
GRID_VIEWS = {"64x64x16": ((4096, 4096), {}), "64x1x16": ((4096, 64), {}), "1x64x16": ((64, 4096), {}), "2x1x16 of 65 x 1": ((65, 1), {}),
              "orthographic 30x17x16": ((1920, 1080), {"is_ortho": True, "ortho_size": 150.0})}


@pytest.mark.parametrize("name", list(GRID_VIEWS))
def test_grid_shapes(ctx, name):
    """The largest grid (65536 clusters: 16 sweeps of the count and fill grids, 64 clusters per thread of the offsets step, the packed
    range byte hi + 1 = 65), a one-row and a one-column grid, a viewport of one pixel row, an orthographic view."""
    (w, h), kw = GRID_VIEWS[name]
    sc = CO.scene()
    view = CO.view(w, h, **kw)
    probes = {k: sc[k] for k in ("env", "env_entities", "refl", "refl_entities")}
    listed = np.random.default_rng(51).choice(CO.N_ENTITIES, 300, replace=False).astype(np.int32)
    wide = np.flatnonzero(sc["lights"]["range"] == np.float32(2.0e4))
    listed[[0, 150, 299]] = wide[:3]  # scene-wide lights at the list's ends and in its middle
    assert len(set(listed.tolist())) == 300
    want = CO.fill_clusters(view, listed, sc["transforms"], sc["lights"], sc["atlas"], **probes)
    size = want["size"]
    assert size == ((w + 63) // 64, (h + 63) // 64, 16)
    rg, radius = want["ranges"], want["lights"]["radius"]
    everywhere = (rg[:, :, 0] == 0).all(axis=1) & (rg[:, :, 1] == size).all(axis=1)
    nowhere = (rg[:, :, 0] == -1).any(axis=1)
    assert (everywhere & (radius == np.float32(2.0e4))).any() and nowhere.sum() > 20 and ((radius < 0.5) & (radius > 0) & ~nowhere).any()
    if name == "64x64x16":
        assert len(want["clusters"]) == 65536 and (rg[:, 0] == (0, 64)).all(axis=1).any() and (rg[:, 1] == (0, 64)).all(axis=1).any()  # the packed byte 65
    _, xp, yp, _ = CO.planes(view["frustum"][0], w, h)
    for pl in (xp, yp):  # an orthographic view's x planes share one normal bit for bit, and so do its y planes; a perspective view's fan out
        assert (len({tuple(r) for r in pl[:, :3].view(np.uint32).tolist()}) == 1) == bool(kw.get("is_ortho"))
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes, map_capacity=max(BIG, len(want["map"])))
    cf.runList(view, listed)
    assert_run_matches(cf, want, name)


# ---- a list beyond one sweep of the record step -----------------------------------------------------------------------------------
def test_list_beyond_one_sweep_of_the_record_step(ctx):
    """CLUSTER_REC_GRID * CLUSTER_BLOCK = 65536 list entries are one sweep of k_cluster_records: 257 more, with scene-wide lights on the
    last entry of the first sweep, the first of the second and the last of the list."""
    sweep = api.CLUSTER_REC_GRID * api.CLUSTER_BLOCK
    n = sweep + 257
    assert sweep == 65536
    sc = CO.scene(n_entities=n)
    rng = np.random.default_rng(61)
    listed = rng.permutation(n).astype(np.int32)
    lights = sc["lights"].copy()
    tiny = rng.random(n) < 0.97  # mostly tiny or outside: the map stays small
    lights["range"][tiny] = rng.uniform(0.01, 0.3, tiny.sum())
    at = [sweep - 1, sweep, n - 1]
    lights["range"][listed[at]] = 2.0e4
    view = CO.view(128, 64)
    want = CO.fill_clusters(view, listed, sc["transforms"], lights, sc["atlas"])
    assert len(want["lights"]) == n and len(want["map"]) < BIG
    for c in (0, len(want["clusters"]) // 2, len(want["clusters"]) - 1):
        assert set(at) <= set(segments(want, c)[0])
    behind = want["ranges"][sweep:]
    assert ((behind[:, :, 1] > behind[:, :, 0]).all(axis=1)).sum() > 3  # lights of the second sweep that land in clusters
    cf = filler(ctx, sc["transforms"], lights, sc["atlas"], max_lights=n)
    cf.runList(view, listed)
    assert_run_matches(cf, want, "beyond one sweep")
    assert cf.readLightEntities().tolist() == listed.tolist()


# ---- the saturating prefix --------------------------------------------------------------------------------------------------------
def test_offsets_saturate_at_2_32_minus_1(ctx):
    """65536 clusters x (65536 lights + 16 environment probes) each: the sum passes 2^32. k_cluster_offsets' hand-written saturating scan
    gives min(c * 65552, 2^32 - 1), and nothing is written to a map of 1024 entries. The expected values are closed-form: the oracle
    cannot hold a map of 2^32 entries."""
    import os

    if os.environ.get("LMX_HOSTSIM") == "1":
        pytest.skip("4 * 10^9 range tests: hours on the simulated device")
    n_lights, n_env, cap = 65536, 16, 1024
    sc = CO.scene(n_entities=n_lights)
    lights = sc["lights"].copy()
    lights["range"] = 1.0e5
    probes = CO.probe_tables(n_env, 0, seed=71, n_entities=n_lights, wide=range(n_env), far=0.0)
    view = CO.view(4096, 4096)
    size, xp, yp, zp = CO.planes(view["frustum"][0], 4096, 4096)
    listed = np.arange(n_lights, dtype=np.int32)
    rec = CO.light_records(listed, sc["transforms"], lights, None, CAM)
    assert (CO.ranges(size, xp, yp, zp, rec["pos"], rec["radius"]) == [[0, 64], [0, 64], [0, 16]]).all()  # every light in every cluster
    e_rec, e_rad = CO.env_probe_records(probes["env"], probes["env_entities"], sc["transforms"], CAM)
    assert len(e_rec) == n_env and (CO.ranges(size, xp, yp, zp, e_rec["pos"], e_rad) == [[0, 64], [0, 64], [0, 16]]).all()
    cf = filler(ctx, sc["transforms"], lights, None, {"env": probes["env"], "env_entities": probes["env_entities"]}, max_lights=n_lights, map_capacity=cap)
    prefill_map(cf, cap)
    cf.runList(view, listed)
    assert cf.counts() == {"lights": n_lights, "env_probes": n_env, "refl_probes": 0, "map_entries": 0xFFFFFFFF, "overflow": 2}
    clusters, got_size = cf.readClusters()
    assert got_size == (64, 64, 16)
    per = n_lights + n_env
    offset = np.minimum(np.arange(65536, dtype=np.uint64) * per, 0xFFFFFFFF).astype(np.uint32)
    assert offset[65520] == 65520 * per < 0xFFFFFFFF and (offset[65521:] == 0xFFFFFFFF).all()  # saturated ones and others
    want = np.zeros(65536, api.CLUSTER)
    want["offset"], want["lights_count"], want["env_probes_count"] = offset, n_lights, n_env
    same_bytes(clusters, want, "saturated clusters")
    guard_words = api.CLUSTERS_GUARD_BYTES // 4
    assert (cf.readMap(cap + guard_words).view(np.uint8) == 0xA5).all(), "no segment fits: the map and its guard are as they were"


# ---- overflow in the middle of the map --------------------------------------------------------------------------------------------
def prefill_map(cf, n_words):
    """0xA5 into the first n_words of the map (the reserve writes them behind the capacity only), through the device pointer"""
    import ctypes as C

    from tests.conftest import hostsim_active

    cf.ctx.synchronize()
    ptr = cf.deviceOutputs()["map"]
    if not n_words:
        return
    if hostsim_active():  # the simulated device's memory is the host's
        C.memset(ptr, 0xA5, 4 * n_words)
    else:  # the HIP runtime the library itself is linked to (already loaded into this process)
        hip = C.CDLL(next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l))
        assert hip.hipMemset(C.c_void_p(ptr), C.c_int(0xA5), C.c_size_t(4 * n_words)) == 0
        assert hip.hipDeviceSynchronize() == 0


def test_overflow_in_the_middle_writes_the_fitting_segments_only(ctx):
    """map_capacity at the start of a cluster in the middle of the grid, one entry short of that cluster's end, and 0: every segment that
    ends at or before the capacity is the oracle's, no word at or past the end of the last fitting segment is written, counts and
    `clusters` are the full ones."""
    sc = CO.scene()
    view, listed, probes, want = seeded_case()
    n, need = len(listed), len(want["map"])
    cl = want["clusters"]
    mid = len(cl) // 2
    total = cl["lights_count"] + cl["env_probes_count"] + cl["refl_probes_count"]
    assert total[mid] > 1 and 0 < cl["offset"][mid] < need
    guard_words = api.CLUSTERS_GUARD_BYTES // 4
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes, max_lights=n)
    for cap in (int(cl["offset"][mid]), int(cl["offset"][mid] + total[mid] - 1), 0):
        cf.reserve(n, cap)
        prefill_map(cf, cap)
        cf.runList(view, listed)
        cnt = cf.counts()
        assert cnt == {"lights": n, "env_probes": len(want["env_probes"]), "refl_probes": len(want["refl_probes"]), "map_entries": need, "overflow": 2}, (cap, cnt)
        same_bytes(cf.readClusters()[0], cl, f"capacity {cap}: clusters")
        same_bytes(cf.readLights(), want["lights"], f"capacity {cap}: lights")
        fits = cl["offset"].astype(np.int64) + total <= cap
        end = int((cl["offset"][fits].astype(np.int64) + total[fits]).max()) if fits.any() else 0
        assert end == (int(cl["offset"][mid]) if cap else 0) and fits.sum() == (mid if cap else 0)  # the clusters in front of `mid`, whole
        got = cf.readMap(cap + guard_words)
        same_bytes(got[:end], want["map"][:end], f"capacity {cap}: the fitting segments")
        assert (got[end:].view(np.uint8) == 0xA5).all(), f"capacity {cap}: words behind the last fitting segment, or the guard, were written"


# ---- a shorter run after a longer one ---------------------------------------------------------------------------------------------
def test_shorter_run_after_a_longer_one(ctx):
    """The second and third run meet the first one's ranges, totals, offsets, records and map behind their own ends."""
    sc = CO.scene()
    view, listed, probes, want = seeded_case()
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes)
    cf.runList(view, listed)
    assert_run_matches(cf, want, "the long run")
    cf.setProbes()
    small = CO.view(128, 64)
    few = listed[100:170]
    want2 = CO.fill_clusters(small, few, sc["transforms"], sc["lights"], sc["atlas"])
    assert len(want2["clusters"]) == 32 < len(want["clusters"]) and 0 < len(want2["map"]) < len(want["map"]) and not len(want2["env_probes"])
    cf.runList(small, few)
    assert_run_matches(cf, want2, "70 lights, no probes, after the long run")
    none = np.zeros(0, np.int32)
    want3 = CO.fill_clusters(small, none, sc["transforms"], sc["lights"], sc["atlas"])
    assert not len(want3["map"]) and not want3["clusters"].view(np.uint32).any()
    cf.runList(small, none)
    assert_run_matches(cf, want3, "an empty list after the two")


# ---- transforms read from the world hierarchy -------------------------------------------------------------------------------------
def test_transforms_from_the_world_follow_its_edits():
    """lmx_draw_bind_world: the records and the binning read the propagated hierarchy in place, and go on doing so after a
    World.edit that renumbers the slots - without a re-bind."""
    from lumixengine_amd import scenes

    own = api.Context(0)
    try:
        h = scenes.hierarchy_chains(40, 3, seed=4, root_extent=60.0)
        n = len(h["parent"])
        cam = (0.0, 0.0, 150.0)
        view = CO.view(128, 64, cam_pos=cam)
        w = api.World(own)
        w.build(h["parent"], h["local"])
        w.propagate()
        dc = api.DrawCommands(own)
        dc.bindWorld(True)
        rng = np.random.default_rng(81)
        lights = np.zeros(n + 2, api.POINT_LIGHT)  # (the entity the edit creates has its record already)
        lights["color"], lights["intensity"] = rng.uniform(0, 1, (n + 2, 3)), rng.uniform(1, 5, n + 2)
        lights["range"] = np.exp(rng.uniform(np.log(0.5), np.log(80.0), n + 2))
        lights["fov"], lights["attenuation_param"] = 1.0, 2.0
        created, leaf, middle, moved, root = n, n - 1, 45, 50, 3  # (45 is the child of root 5 and the parent of 85; 50 the child of root 10)
        assert h["parent"][middle] == 5 and h["parent"][85] == middle and h["parent"][moved] == 10 and h["parent"][root] < 0
        lights["range"][[created, moved, 85]] = 2.0e4
        probes = {"env": np.zeros(5, api.ENV_PROBE), "env_entities": np.array([created, leaf, 85, moved, 7], np.int32),
                  "refl": np.zeros(4, api.REFL_PROBE), "refl_entities": np.array([middle, created, 20, root], np.int32)}
        probes["env"]["outer_range"] = rng.uniform(20, 100, (5, 3))
        probes["env"]["inner_range"] = probes["env"]["outer_range"] * np.float32(0.5)
        probes["env"]["flags"] = api.PROBE_ENABLED
        probes["refl"]["half_extents"] = rng.uniform(20, 100, (4, 3))
        probes["refl"]["flags"] = api.PROBE_ENABLED
        listed = np.concatenate([rng.permutation(n)[:60], [created, leaf, middle, 85, moved]]).astype(np.int32)
        cf = api.ClusterFiller(own)
        cf.setLights(lights)
        cf.setAtlas(None)
        cf.setProbes(**probes)
        cf.reserve(256, BIG)
        cf.runList(view, listed)
        before = w.getTransforms()
        want = CO.fill_clusters(view, listed, before, lights, None, **probes)
        assert len(want["map"]) > 100 and (want["lights"]["pos"][: 60] != 0).any()
        assert not want["lights"]["rot"][list(listed).index(created)].any()  # not in the world yet: reads as zero
        assert_run_matches(cf, want, "the world as built")
        # destroy a leaf and a node in the middle of a chain (its subtree goes with it), create an entity, re-parent a child to another root
        w.edit(destroy=[leaf, middle], create=[created], create_transforms=scenes.random_transforms(rng, 1, 30.0), reparent=[(root, moved)])
        w.setTransforms(np.array([root, 10], np.int32), scenes.random_transforms(rng, 2, 40.0))
        w.propagate()
        info = w.info()
        assert info["edits"] == 1 and info["n"] == n + 1 and info["n_live"] == n + 1 - 3
        cf.runList(view, listed)  # no bindWorld, no setTransforms in between
        after = w.getTransforms()
        assert len(after) == n + 1 and after[moved].tobytes() != before[moved].tobytes() and after[created]["rot"].any()
        want = CO.fill_clusters(view, listed, after, lights, None, **probes)
        assert want["lights"].tobytes() != CO.light_records(listed, before, lights, None, cam).tobytes()
        for c in (0, 31):
            assert {list(listed).index(created), list(listed).index(moved)} <= set(segments(want, c)[0])
        assert_run_matches(cf, want, "after the edit")
    finally:
        own.close()
