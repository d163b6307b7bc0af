"""The engine-facing adapters of lumixengine_amd/host/ RUN, not only compiled: C++ drivers (tests/cpp/run_*.cpp) read a scenario written
here, fill the in-memory mocks of tests/cpp/lumix_compat*.h, drive an adapter through its public methods in the order its header gives for
an engine frame and write what the engine would consume; the result is compared with the oracle the direct-ABI test of that subsystem
uses, fed the same calls. An adapter only marshals, so every comparison is bit for bit (NaN payloads canonicalised as canon() of
tests/test_gpu_instanced_models.py does). Runs on the MI355X and under `pytest -m gpu --hostsim`.

Adapters run: GpuInstancedModels, GpuClusterFiller (chained behind GpuCullingSystem) and GpuGrass in this file, GpuRayCaster in
tests/test_gpu_adapters_run_rays.py, GpuAnimatorControllers / GpuAnimators in tests/test_gpu_adapters_run_animators.py, GpuParticleSystems in
tests/test_gpu_adapters_run_particles.py (each with its own method -> test table). Still compile-only (tests/test_*_compile.py):
GpuDrawEncoder::encode (needs the engine's draw stream, exists only under LMX_WITH_LUMIX_HEADERS), GpuDrawEncoder::run and GpuPoseProcessor
(one-call forwards whose set-up - key run, sort - would have to be rebuilt in C++ for no new logic).

A driver ends with a step's own exit status when an adapter call answers `false` where the scenario says `true`, or the reverse, and prints
lastError() (tests/cpp/adapter_run.h).

Public method -> test (lastError() / handle() are read by every driver on its error paths):

  GpuInstancedModels::endInstancedModelEditing, slotOf, entities      test_instanced_models_registry_origins_and_destroy
  GpuInstancedModels::setOrigin, flushOrigins, encodeInstancedModels  test_instanced_models_registry_origins_and_destroy
  GpuInstancedModels::destroyInstancedModel, deviceOutputs            test_instanced_models_registry_origins_and_destroy
  GpuClusterFiller::setLights, setProbes, setAtlas, reserve, fill     test_cluster_filler_behind_a_cull
  GpuClusterFiller::counts, deviceOutputs                             test_cluster_filler_behind_a_cull, ..._overflow_then_larger_reserve
  GpuGrass::setTerrains, createGrass, invalidate, cull, getDraws      test_grass_two_terrains_two_frames
  GpuGrass::createGrass returning false                               test_grass_pool_one_slot_short
"""
import struct

import numpy as np
import pytest

from lumixengine_amd import api
from tests import cluster_oracle as CO
from tests import grass_oracle as GO
from tests import im_oracle as IO
from tests.adapters_run import DRIVERS, Out, build_exe, library, raw, run_driver, u32
from tests.test_gpu_instanced_models import canon


@pytest.mark.parametrize("name", ["run_instanced_models", "run_cluster_filler", "run_grass"])
def test_driver_compiles_and_links(name):
    library()
    assert name in DRIVERS and build_exe(name)


# ---- GpuInstancedModels against tests/im_oracle.py -----------------------------------------------------------------------------------
class ImScript:
    """The steps of run_instanced_models.cpp and the oracle, fed the same calls. The oracle's model index is the adapter's slot: the order in
    which entities were first edited."""
    EDIT, ORIGIN, ENCODE, DESTROY, FLUSH, SLOT_OF = 1, 2, 3, 4, 5, 6

    def __init__(self):
        self.steps, self.checks = [], []
        self.orc = IO.Oracle()
        self.slots = []  # entity of every slot
        self.origins = []

    def edit(self, entity, lod_dist, lod_idx, radius, indices, inst):
        inst = np.ascontiguousarray(inst, IO.IM_INSTANCE)
        self.steps.append(u32(self.EDIT) + struct.pack("<i", entity) + raw(lod_dist, np.float32) + raw(lod_idx, np.int32) + struct.pack("<fI", radius, len(indices)) +
                          raw(indices, np.uint32) + u32(len(inst)) + inst.tobytes() + u32(1))
        if entity not in self.slots:
            self.slots.append(entity)
            self.origins.append([0.0, 0.0, 0.0])
        m = self.slots.index(entity)
        self.orc.set_model(m, lod_dist, lod_idx, radius, indices)
        self.orc.set_instances(m, inst)

    def origin(self, entity, pos):
        self.steps.append(u32(self.ORIGIN) + struct.pack("<i", entity) + raw(pos, np.float64))
        if entity in self.slots:
            self.origins[self.slots.index(entity)] = list(pos)

    def flush(self):
        self.steps.append(u32(self.FLUSH))

    def destroy(self, entity, known=True):
        self.steps.append(u32(self.DESTROY) + struct.pack("<i", entity) + u32(int(known)))
        if known:
            self.orc.set_instances(self.slots.index(entity), np.zeros(0, IO.IM_INSTANCE))

    def slot_of(self, entity):
        self.steps.append(u32(self.SLOT_OF) + struct.pack("<i", entity))
        want = (self.slots.index(entity) if entity in self.slots else -1, list(self.slots))
        self.checks.append(("slot", entity, want))

    def encode(self, slot, cam, frustum, lod_multiplier, time_delta, is_shadow):
        self.steps.append(u32(self.ENCODE, slot) + raw(cam, np.float64) + raw(frustum, api.SHIFTED_FRUSTUM) + struct.pack("<ffII", lod_multiplier, time_delta, int(is_shadow), 1))
        self.orc.set_origins(self.origins)
        counts, recs, ind = self.orc.run(api.im_view(cam, lod_multiplier, time_delta, is_shadow), frustum)
        inst = [md["inst"].copy() for md in self.orc.models]
        self.checks.append(("encode", len(self.checks), (counts, recs, ind, inst)))
        return counts, recs, ind

    def compare(self, out: Out):
        for kind, what, want in self.checks:
            if kind == "slot":
                assert (out.i32(), out.counted(np.int32).tolist()) == want, f"slotOf({what}) / entities()"
                continue
            counts, recs, ind, inst = want
            got = out.counted(api.IM_COUNTS)
            assert len(got) == len(counts)
            for m, c in enumerate(counts):
                assert list(got[m]["bin_count"]) == c["bin_count"] and list(got[m]["bin_offset"]) == c["bin_offset"], (what, m, got[m], c)
                assert int(got[m]["unplaced"]) == c["unplaced"] and int(got[m]["instances"]) == c["instances"], (what, m, got[m], c)
            assert canon(out.counted(IO.IM_INSTANCE)) == canon(recs), f"encode {what}: bin records"
            assert np.array_equal(out.counted(api.IM_INDIRECT).view(np.uint32).reshape(-1, 5), ind), f"encode {what}: indirect records"
            for m, want_inst in enumerate(inst):
                assert canon(out.counted(IO.IM_INSTANCE)) == canon(want_inst), f"encode {what}: LOD state of slot {m}"
        assert out.done()


def _im_field(rng, n, half):
    from tests.test_gpu_instanced_models import field

    return field(rng, n, half)


@pytest.mark.gpu
def test_instanced_models_registry_origins_and_destroy(tmp_path):
    from tests.test_gpu_instanced_models import LOD_IDX_4, cascades, main_view

    rng = np.random.default_rng(31)
    s = ImScript()
    lod_dist = [100.0, 900.0, 4000.0, 20000.0]
    # three entities out of numeric order: slot 0 = entity 40 (no instance), slot 1 = entity 7 (one, in front of the camera), slot 2 = entity 19
    s.edit(40, lod_dist, LOD_IDX_4, 1.5, [30, 20, 10, 5], np.zeros(0, IO.IM_INSTANCE))
    one = _im_field(rng, 1, 1.0)
    one["pos"], one["lod"], one["scale"] = [0.0, 0.0, 0.0], 0.0, 1.0
    s.edit(7, lod_dist, LOD_IDX_4, 1.0, [7, 5], one)
    s.edit(19, [200.0, 1200.0, 5000.0, 20000.0], LOD_IDX_4, 2.0, [12, 9, 6, 3], _im_field(rng, 9000, 150.0))
    assert s.slots == [40, 7, 19]
    for e in (40, 7, 19, 5):
        s.slot_of(e)
    cam = (0.0, 6.0, 0.0)
    main = main_view(api, cam)
    d = np.array([np.sin(0.3), -0.15, -np.cos(0.3)])
    s.origin(7, list(np.asarray(cam) + 12.0 * d))  # on the main view's axis: the single instance is drawn
    s.origin(19, [-40.0, 1.0, 30.0])
    c_main, recs_main, _ = s.encode(0, cam, main, 1.0, 1 / 60, False)
    assert sum(c_main[0]["bin_count"]) == 0 and sum(c_main[1]["bin_count"]) >= 1 and sum(c_main[2]["bin_count"]) > 100
    s.encode(1, cam, cascades(api, cam)[2], 1.0, 1 / 60, True)
    # setOrigin alone, then encode: the origin has taken effect (the oracle's records move with it)
    s.origin(19, [25.0, 0.0, -60.0])
    c_moved, recs_moved, _ = s.encode(0, cam, main, 1.0, 1 / 60, False)
    assert c_moved[2]["bin_count"] != c_main[2]["bin_count"] and sum(c_moved[2]["bin_count"]) > 100
    # ... and through the ray caster's flush, which leaves nothing for the next encode to upload
    s.origin(40, [3.0, 0.0, 3.0])
    s.origin(19, [10.0, 0.0, 5.0])
    s.flush()
    s.encode(0, cam, main, 1.0, 1 / 30, False)
    # destroyInstancedModel keeps the slot: no count, indirect records of 0 instances, the others' LOD state as the oracle's
    s.destroy(7)
    c_gone, _, ind_gone = s.encode(0, cam, main, 1.0, 1 / 60, False)
    assert sum(c_gone[1]["bin_count"]) == 0 and c_gone[1]["instances"] == 0 and len(ind_gone) == 4 + 2 + 4 and (ind_gone[4:6, 1] == 0).all()
    assert sum(c_gone[2]["bin_count"]) > 100
    s.slot_of(7)
    # the entity edited again takes the same slot
    s.edit(7, lod_dist, LOD_IDX_4, 1.0, [7, 5], _im_field(rng, 3000, 40.0))
    assert s.slots == [40, 7, 19]
    s.slot_of(7)
    c_back, _, _ = s.encode(0, cam, main, 1.0, 1 / 60, False)
    assert sum(c_back[1]["bin_count"]) > 50
    # an entity nobody registered: destroy answers false, setOrigin is a no-op
    s.destroy(1234, known=False)
    s.origin(1234, [1e6, 1e6, 1e6])
    s.slot_of(1234)
    s.encode(0, cam, main, 1.0, 1 / 60, False)
    s.encode(1, cam, cascades(api, cam)[1], 1.0, 1 / 60, True)
    s.compare(run_driver("run_instanced_models", tmp_path, b"".join(s.steps)))


# ---- GpuClusterFiller behind GpuCullingSystem against tests/cluster_oracle.py --------------------------------------------------------
N_CLUSTER_ENTITIES = 600
LIGHT_IN = np.dtype([("entity", "<i4"), ("color", "<f4", 3), ("intensity", "<f4"), ("range", "<f4"), ("fov", "<f4"), ("attenuation_param", "<f4"), ("flags", "<u4")])
CULLED = np.dtype([("entity", "<i4"), ("type", "<u4"), ("radius", "<f4")])


def cluster_case():
    """The first 600 entities of the cluster oracle's scene: a sparse subset of them are PointLights (in a shuffled module order), one more
    PointLight sits on an entity past the range, the probes (disabled ones among them) sit on entities of the range."""
    sc = CO.scene()
    n = N_CLUSTER_ENTITIES
    rng = np.random.default_rng(19)
    light_entities = rng.permutation(n)[:230].astype(np.int32)
    table = np.zeros(n, api.POINT_LIGHT)  # what the oracle reads: by entity, zero where there is no light
    table[light_entities] = sc["lights"][light_entities]
    module_lights = np.zeros(len(light_entities) + 1, LIGHT_IN)
    order = np.insert(light_entities, 57, 650)  # the PointLight of entity 650 >= n_entities: skipped
    module_lights["entity"] = order
    for k in api.POINT_LIGHT.names:
        module_lights[k] = sc["lights"][order][k]
    env_entities = rng.choice(n, len(sc["env"]), replace=False).astype(np.int32)
    refl_entities = rng.choice(n, len(sc["refl"]), replace=False).astype(np.int32)
    culled = np.zeros(n, CULLED)
    culled["entity"] = np.arange(n)
    is_light = np.zeros(n, bool)
    is_light[light_entities] = True
    culled["type"] = np.where(is_light, 2, 0)  # LOCAL_LIGHT and MESH
    culled["radius"] = np.where(is_light, np.maximum(table["range"], 0.01), 1.0)
    view = CO.view(640, 360)
    probes = {"env": sc["env"], "env_entities": env_entities, "refl": sc["refl"], "refl_entities": refl_entities}
    return sc["transforms"][:n], table, module_lights, sc["atlas"][:n], probes, culled, view, light_entities


def cluster_scenario(max_lights=4096, map_capacity=1 << 20):
    tr, table, module_lights, atlas, probes, culled, view, _ = cluster_case()
    v = view.reshape(-1)[0]
    return b"".join([u32(len(tr)), tr.tobytes(), u32(len(module_lights)), module_lights.tobytes(),
                     u32(len(probes["env"])), raw(probes["env"], api.ENV_PROBE), raw(probes["env_entities"], np.int32),
                     u32(len(probes["refl"])), raw(probes["refl"], api.REFL_PROBE), raw(probes["refl_entities"], np.int32),
                     raw(atlas, np.uint32), u32(len(culled)), culled.tobytes(), raw(v["frustum"], api.SHIFTED_FRUSTUM), raw(v["camera_pos"], np.float64),
                     u32(int(v["viewport_w"]), int(v["viewport_h"]), max_lights, map_capacity)])


def read_cluster_run(out: Out):
    counts = out.arr(api.CLUSTERS_COUNTS, 1)[0]
    visible = out.counted(np.int32)
    if counts["overflow"]:
        return counts, visible, None
    size = tuple(int(x) for x in out.arr(np.uint32, 3))
    n = int(counts["lights"])
    got = {"size": size, "lights": out.arr(api.CLUSTER_LIGHT, n), "entities": out.arr(np.int32, n), "clusters": out.arr(api.CLUSTER, size[0] * size[1] * size[2]),
           "map": out.arr(np.int32, int(counts["map_entries"])), "env_probes": out.arr(api.CLUSTER_ENV_PROBE, int(counts["env_probes"])),
           "refl_probes": out.arr(api.CLUSTER_REFL_PROBE, int(counts["refl_probes"]))}
    return counts, visible, got


def assert_clusters_match(counts, visible, got, what):
    tr, table, _, atlas, probes, _, view, light_entities = cluster_case()
    listed = got["entities"]
    # the list is the cull's: the LOCAL_LIGHT ids the CullingSystem interface returned for the same frustum, and lights only
    assert sorted(listed.tolist()) == sorted(visible.tolist()) and set(listed.tolist()) <= set(light_entities.tolist()), what
    assert 20 < len(listed) < len(light_entities), what
    want = CO.fill_clusters(view, listed, tr, table, atlas, **probes)
    assert {k: int(counts[k]) for k in api.CLUSTERS_COUNTS.names} == {"lights": len(want["lights"]), "env_probes": len(want["env_probes"]), "refl_probes": len(want["refl_probes"]),
                                                                    "map_entries": len(want["map"]), "overflow": 0}, what
    assert got["size"] == want["size"], what
    assert len(want["env_probes"]) == 7 and len(want["refl_probes"]) == 6  # the disabled ones are left out
    for k in ("lights", "clusters", "map", "env_probes", "refl_probes"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"{what}: {k} differ"
    return want


@pytest.fixture(scope="module")
def cluster_runs(tmp_path_factory):
    """the driver's three runs, taken once: [(counts, the cull's LOCAL_LIGHT ids, buffers or None)]"""
    out = run_driver("run_cluster_filler", tmp_path_factory.mktemp("clusters"), cluster_scenario())
    runs = [read_cluster_run(out) for _ in range(3)]
    assert out.done()
    return runs


@pytest.mark.gpu
def test_cluster_filler_behind_a_cull(cluster_runs):
    counts, visible, got = cluster_runs[0]
    want = assert_clusters_match(counts, visible, got, "generous reserve")
    # the tables carried something: lights with and without an atlas slot, clusters that hold lights and both kinds of probes
    assert (want["lights"]["atlas_idx"] == 0xFFFFFFFF).any() and (want["lights"]["atlas_idx"] != 0xFFFFFFFF).any()
    cl = want["clusters"]
    assert ((cl["lights_count"] > 0) & (cl["env_probes_count"] > 0) & (cl["refl_probes_count"] > 0)).any()


@pytest.mark.gpu
def test_cluster_filler_overflow_then_larger_reserve(cluster_runs):
    """the driver's second run reserves one light record fewer than the first run listed: counts() sets overflow bit 0 and names the sizes a
    larger reserve needs; the third run reserves exactly those and matches"""
    first = cluster_runs[0][0]
    counts, visible, got = cluster_runs[1]
    assert got is None and int(counts["overflow"]) == 1 and int(counts["lights"]) == int(first["lights"]) and int(counts["map_entries"]) == int(first["map_entries"])
    counts, visible, got = cluster_runs[2]
    assert_clusters_match(counts, visible, got, "after the larger reserve")


# ---- GpuGrass against tests/grass_oracle.py ------------------------------------------------------------------------------------------
TEXTURE_FORMAT = {"R8": 0, "RGBA8": 1, "R16": 2}  # gpu::TextureFormat of tests/cpp/lumix_compat_grass.h
GRASS_CREATE, GRASS_INVALIDATE, GRASS_CULL = 1, 2, 3


def grass_case():
    """Four terrains at non-zero world positions, two types each: an RGBA8 heightmap; an R16 one; one without a splat map (createGrass makes
    nothing of it); one whose splat map is not RGBA8 (the quads exist and are empty). -> (terrains, positions, splat formats)"""
    from tests.test_gpu_grass import ALL_RANDOM, Y_UP, grid_distance, heightmap, splat_random, terrain

    two = [(0.5, grid_distance(0.5, 2), Y_UP, 1), (0.75, grid_distance(0.75, 1), ALL_RANDOM, 1)]
    loading = [(0.5, grid_distance(0.5, 1), ALL_RANDOM, 0), (0.75, grid_distance(0.75, 2), Y_UP, 1)]  # type 0's model is not ready: cached, never drawn
    terrains = [terrain("adapter rgba8", heightmap(64, 64, np.uint32, 31), splat_random(64, 64, 0.3, 32, bits=0x3), two, scale=(1.0, 25.0, 1.0), entity=3),
                terrain("adapter r16", heightmap(48, 80, np.uint16, 33), splat_random(48, 80, 0.3, 34, bits=0x3), loading, scale=(2.0, 12.0, 2.0), entity=9),
                terrain("adapter no splat", heightmap(32, 32, np.uint16, 35), None, two, entity=1, splat_ready=False),
                terrain("adapter r8 splat", heightmap(32, 32, np.uint16, 36), splat_random(32, 32, 0.5, 37, bits=0x3), two[:1] + [(0.0, 10.0, Y_UP, 1)], entity=6,
                        splat_format=0xFFFFFFFF)]
    positions = np.array([[120.0, -4.0, 64.0], [131.0, 2.5, 22.0], [100.0, 0.0, 50.0], [90.0, 1.0, 70.0]])
    return terrains, positions, ["RGBA8", "RGBA8", None, "R8"]


def grass_header(n_slots):
    terrains, positions, splat_formats = grass_case()
    parts = [u32(n_slots, len(terrains))]
    for t, pos, sf in zip(terrains, positions, splat_formats):
        hm = np.ascontiguousarray(t["heightmap"])
        parts += [struct.pack("<i", t["entity"]), raw(pos, np.float64), struct.pack("<ii", hm.shape[1], hm.shape[0]), raw(t["scale"], np.float32),
                  u32(TEXTURE_FORMAT["R16" if hm.dtype == np.uint16 else "RGBA8"]), hm.tobytes()]
        if t["splatmap"] is None:
            parts.append(u32(0))
        else:
            sp = np.ascontiguousarray(t["splatmap"], np.uint32)
            parts += [u32(1, sp.shape[1], sp.shape[0], TEXTURE_FORMAT[sf]), sp.tobytes()]
        parts.append(u32(len(t["types"])))
        for k, (spacing, distance, mode, usable) in enumerate(t["types"]):
            parts.append(struct.pack("<ffiI", spacing, distance, mode, 1 if usable else 2 * (k % 2 == 0)))  # not usable: a model still loading, or none
    return b"".join(parts)


def grass_centres(positions, cam):
    """renderGrass's centre of every terrain: Vec2(-(float)rel.x, -(float)rel.z) of the terrain's position relative to the camera"""
    rel = np.asarray(positions, np.float64) - np.asarray(cam, np.float64)
    return [(-np.float32(r[0]), -np.float32(r[2])) for r in rel]


def grass_views(cam):
    from tests.test_gpu_grass import EVERYTHING, view

    return np.array([view(api.frustum_perspective(cam, np.float32([0.5, -0.2, 0.84]), (0, 1, 0), 1.1, 1.5, 0.1, 200.0)[0], cam),
                     view(api.frustum_ortho(np.asarray(cam) + (0.0, 50.0, 0.0), (-0.1, 0.98, -0.1), (0, 0, 1), 25.0, 25.0, 0.0, 120.0)[0], cam, 2.0),  # (looks along -direction: down)
                     view(EVERYTHING, cam, 4.0)], api.GRASS_VIEW)


def grass_create_step(cam, frame, expect=True):
    return u32(GRASS_CREATE) + raw(cam, np.float64) + u32(frame, int(expect))


def grass_cull_step(views):
    return u32(GRASS_CULL, len(views)) + b"".join(raw(v["frustum"], api.SHIFTED_FRUSTUM) + raw(v["viewport_pos"], np.float64) + struct.pack("<f", v["lod_multiplier"]) for v in views)


def check_grass_quads(out: Out, o, what):
    from tests.conftest import hostsim_active

    want = o.records()
    got = out.counted(api.GRASS_QUAD)
    assert got.tobytes() == want.tobytes(), f"{what}: quad records differ\n{got}\n{want}"
    for rec in want:
        inst = out.arr(api.GRASS_INSTANCE, int(rec["instances_count"]))
        q = o.quad(int(rec["terrain"]), int(rec["type"]), int(rec["ij"][0]), int(rec["ij"][1]))["instances"]
        # positions and scales bit for bit; the rotations go through the device's sinf / cosf (tests/test_gpu_grass.py bounds those): bit for
        # bit where both sides call the host's libm
        for k in ("position", "scale") + (("rotation",) if hostsim_active() else ()):
            assert inst[k].tobytes() == q[k].tobytes(), f"{what}: {k} of quad {rec['ij']} type {rec['type']} terrain {rec['terrain']} differs"
    return want


def check_grass_cull(out: Out, terrains, positions, records, views, what):
    want = GO.cull(terrains, positions, records, views)
    for v, (draws, c) in enumerate(want):
        got_c = out.arr(api.GRASS_COUNTS, 1)[0]
        got_d = out.counted(api.GRASS_DRAW)
        assert got_c.tobytes() == c.tobytes(), f"{what}: counts of view {v}: {got_c} vs {c}"
        assert got_d.tobytes() == draws.tobytes(), f"{what}: draws of view {v} differ"
    return want


GRASS_CAMS = ((150.0, 8.0, 92.0), (167.0, 9.0, 85.0))


@pytest.mark.gpu
def test_grass_two_terrains_two_frames(tmp_path):
    terrains, positions, _ = grass_case()
    n_slots = 48
    o = GO.Grass(terrains, n_slots)
    views = [grass_views(cam) for cam in GRASS_CAMS]
    scenario = (grass_header(n_slots) + grass_create_step(GRASS_CAMS[0], 5) + grass_cull_step(views[0]) + u32(GRASS_INVALIDATE, 1) +
                grass_create_step(GRASS_CAMS[1], 6) + grass_cull_step(views[1]))
    out = run_driver("run_grass", tmp_path, scenario)
    # frame 5
    o.update(5, grass_centres(positions, GRASS_CAMS[0]))
    first = check_grass_quads(out, o, "frame 5")
    assert set(first["terrain"].tolist()) == {0, 1, 3}  # the terrain without a splat map has no quad
    assert (first["instances_count"][first["terrain"] == 3] == 0).all() and (first["instances_count"][first["terrain"] == 0] > 0).any()
    want = check_grass_cull(out, terrains, positions, first, views[0], "frame 5")
    assert all(int(c["draws"]) > 0 for _, c in want) and any(int(c["culled"]) > 0 for _, c in want)
    drawn = {(int(d["terrain"]), int(d["type"])) for d in want[2][0]}
    assert {(0, 0), (0, 1), (1, 1)} <= drawn and (1, 0) not in drawn  # both terrains' quads are placed where the views see them; a loading model draws nothing
    # invalidate(1), then frame 6 with the camera a quad further: terrain 1's quads are made again in the slots it freed, the others' are kept or new
    o.invalidate(1)
    created = o.update(6, grass_centres(positions, GRASS_CAMS[1]))
    assert {c[0] for c in created} >= {0, 1} and len(created) < len(o.live())
    second = check_grass_quads(out, o, "frame 6")
    assert second.tobytes() != first.tobytes()
    check_grass_cull(out, terrains, positions, second, views[1], "frame 6")
    assert out.done()


@pytest.mark.gpu
def test_grass_pool_one_slot_short(tmp_path):
    terrains, positions, _ = grass_case()
    centres = grass_centres(positions, GRASS_CAMS[0])
    need = len(GO.Grass(terrains, 64).update(5, centres))
    with pytest.raises(GO.CapacityError):
        GO.Grass(terrains, need - 1).update(5, centres)
    out = run_driver("run_grass", tmp_path, grass_header(need - 1) + grass_create_step(GRASS_CAMS[0], 5, expect=False))
    assert len(out.counted(api.GRASS_QUAD)) == 0 and out.done()  # createGrass answered false and nothing was cached: the engine runs its own loop this frame
    # the same frame with exactly enough slots; and a scenario that expects `true` of the short pool ends the driver with that step's exit code
    out = run_driver("run_grass", tmp_path, grass_header(need) + grass_create_step(GRASS_CAMS[0], 5))
    o = GO.Grass(terrains, need)
    o.update(5, centres)
    check_grass_quads(out, o, "exactly enough slots")
    run_driver("run_grass", tmp_path, grass_header(need - 1) + grass_create_step(GRASS_CAMS[0], 5), expect_rc=10 + GRASS_CREATE)
