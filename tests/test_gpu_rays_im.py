"""Instanced models in the device ray cast (lmx_rays_set_instanced_models, k_imray_* of ray_kernels.hip) against tests/ray_im_oracle.py, bit
for bit: every field of LmxRayImHit and of LmxRayHit, and both stages' candidate counts. One instance and one triangle (hit, sphere miss,
origin inside the sphere, t < 0, identity and quarter-turn quaternions, scales 0.5 / 3 / negative), t_max around the hit, the three ways a
model is skipped, ties between twin instances (same wave, next wave, next 256-slot tile, across models), model sizes and nearest instances
on every wave / tile / IM_TILE edge, padding slots that hold stale instances, shared and distinct ray-table models, a mesh that crosses the
narrow phase's split, the join with the model-instance stage (nearer, farther, equal, a skinned model instance next to its unskinned
instanced copy), ray-tile edges, the golden fixture, overflow, detach, a later lmx_im_set_instances, rays in device memory, the error
codes and an empty batch. Every scene is checked on the CPU first: the reference's walk and the order-free form must agree on it.

Instances that share x and z land in one grid cell and keep their order (the grid build is a stable scatter): the stored order every
scene's oracle uses is read back from the device all the same."""
import os

import numpy as np
import pytest

from lumixengine_amd import api
from tests import ray_im_oracle as RIO
from tests import ray_oracle as RO
from tests.test_gpu_rays import TRI, caster, cube, down, filler, mesh, rig, same_hits, scene_of, seeded, skin_of, transforms

pytestmark = pytest.mark.gpu

f32 = np.float32
EV = api.RAY_INSTANCE_ENABLED | api.RAY_INSTANCE_VALID
CHUNK = api.RAY_BLOCK * api.RAY_RUN
INVALID, CAPACITY, NOT_BUILT = 1, 5, 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRI_Y = [[0, 0, 0], [0, 0, 1], [1, 0, 0]]  # normal +y: met by a ray straight down -y, and x / z (the grid's axes) stay free


LIVE = []  # every InstancedModels of this module: destroyed before the context they belong to (lmx_im_destroy reads it)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    api.RayCaster(c).setInstancedModels(None)
    while LIVE:
        LIVE.pop().close()
    c.close()


def ydown(x, z, y=5.0, **kw):
    return api.rays([[x, y, z]], [[0, -1, 0]], **kw)


def inst(pos, scale=1.0, rot=(0, 0, 0)):
    pos = np.asarray(pos, f32).reshape(-1, 3)
    a = np.zeros(len(pos), api.IM_INSTANCE)
    a["pos"], a["scale"], a["rot"] = pos, scale, rot
    return a


def imodel(ray_model, entity, instances, origin=(0, 0, 0)):
    return {"ray_model": ray_model, "entity": entity, "origin": np.asarray(origin, np.float64), "instances": instances}


def no_entities(model_meshes, **kw):
    """the ray-table models alone: one entity without a model"""
    return scene_of(model_meshes, [-1], transforms([[0, 0, 0]]), **kw)


def attach(ctx, rc, sc, im_models):
    """-> the InstancedModels; sc["im_models"] = the models with their instances in the STORED order and the radius the device holds"""
    im = api.InstancedModels(ctx)
    LIVE.append(im)
    for mdl in im_models:
        rm = mdl["ray_model"]
        mdl["radius"] = f32(sc["models"][rm]["origin_radius"]) if 0 <= rm < len(sc["models"]) else f32(1)
        m = im.addModel([1e8, -1, -1, -1], [(0, 0), (0, -1), (0, -1), (0, -1), (0, -1)], mdl["radius"], [3])
        im.setInstances(m, mdl["instances"])
        mdl["instances"] = im.readInstances(m)
    im.setOrigins([m["origin"] for m in im_models] or np.zeros((0, 3)))
    rc.setInstancedModels(im, [m["ray_model"] for m in im_models], [m["entity"] for m in im_models])
    sc["im_models"] = im_models
    return im


def expect(rc, sc, rays, what):
    assert RIO.agrees(sc, rays), f"{what}: a bad scene - the reference's walk and the order-free form differ"
    want_im, want = RIO.cast_all(sc, rays)
    assert rc.imCounts() == {"rays": len(rays), "candidates": RIO.candidates_im(sc, rays), "overflow": 0}, what
    assert rc.counts() == {"rays": len(rays), "candidates": RO.candidates(sc, RIO.effective_rays(rays, want_im)), "overflow": 0}, what
    same_hits(rc.readImHits(), want_im.astype(api.RAY_IM_HIT), what + " (instanced models)")
    same_hits(rc.readHits(), want.astype(api.RAY_HIT), what + " (model instances)")
    return want_im, want


def check(ctx, sc, im_models, rays, what="", twice=False, **kw):
    rc = caster(ctx, sc, **kw)
    im = attach(ctx, rc, sc, im_models)
    rc.cast(rays)
    want_im, want = expect(rc, sc, rays, what)
    if twice:
        a, b = rc.readImHits().tobytes(), rc.readHits().tobytes()
        rc.cast(rays)
        assert rc.readImHits().tobytes() == a and rc.readHits().tobytes() == b, what + ": two runs differ"
    rc.setInstancedModels(None)
    im.close()
    return want_im, want


# ---- one instance, one triangle -------------------------------------------------------------------------------------------------
def single_scene():
    sc = no_entities([[mesh(TRI_Y)]])
    rays = np.concatenate([
        ydown(0.25, 0.25),                               # a hit, identity quaternion
        ydown(9.0, 0.25),                                # past the sphere
        ydown(0.25, 0.25, y=0.5),                        # the origin inside the sphere: the tca + thc branch
        ydown(0.25, 0.25, y=-0.5),                       # ... below the triangle: the sphere passes, the triangle's t < 0
        ydown(0.25, 0.25, y=-9.0),                       # the sphere behind the origin: sphere t < 0
        ydown(0.75, 0.75),                               # through the sphere, past the triangle
        api.rays([[0.25, -5, 0.25]], [[0, 1, 0]]),       # from below
    ])
    return sc, [imodel(0, 7, inst([[0, 0, 0]]))], rays


def test_single_instance_cases(ctx):
    want_im, _ = check(ctx, *single_scene(), "single instance", twice=True)
    assert want_im["is_hit"].tolist() == [1, 0, 1, 0, 0, 0, 1] and want_im["t"][0] == 5 and want_im["t"][2] == f32(0.5)
    assert want_im["entity"][0] == 7 and want_im["subindex"][0] == 0 and want_im["model"][0] == 0


def rotation_scene():
    """a quarter turn about x lays the triangle into the xy plane (met along -z); scales 0.5 and 3: t = t_model * scale; the model's origin
    far out is taken off in fp64; the entity's own rotation and scale do not exist for the cast"""
    q = f32(np.sqrt(0.5))
    origin = np.array([1.0e6, 50.0, -1.0e6])
    instances = np.concatenate([inst([[0, 0, 0]], 0.5), inst([[10, 0, 0]], 3.0), inst([[20, 0, 0]], 1.0, (q, 0, 0)), inst([[30, 0, 0]], 2.0, (0.3, -0.2, 0.5))])
    sc = no_entities([[mesh(TRI_Y)]])
    general = np.array([0.3, -0.2, 0.5, np.sqrt(1 - 0.38)], f32)
    centre = f32([30, 0, 0]) + RO._rotate(general, f32([1 / 3, 0, 1 / 3]) * f32(2), f32)  # the fourth instance's triangle, in the model's frame
    rays = np.concatenate([ydown(0.1, 0.1), ydown(10.5, 0.5), api.rays([[20.25, -0.25, 5]], [[0, 0, -1]]), ydown(centre[0], centre[2]),
                           api.rays([centre + f32([0, 4, 3])], [[0, -0.8, -0.6]])])
    rays["origin"] += origin
    return sc, [imodel(0, 3, instances, origin)], rays


def test_rotation_scale_and_origin(ctx):
    want_im, _ = check(ctx, *rotation_scene(), "rotation and scale")
    assert want_im["is_hit"].tolist() == [1, 1, 1, 1, 1]
    assert want_im["t_model"][0] == 10 and want_im["t"][0] == 5 and want_im["t"][1] == 5 and abs(want_im["t"][2] - 5) < 1e-5


def negative_scene(second=False):
    sc = no_entities([[mesh(TRI_Y)]])
    if second:
        instances = np.concatenate([inst([[0, 0, 0]], -1.0), inst([[0, 0.25, 0]], -1.0), inst([[0, -3, 0]], 1.0)])
    else:
        instances = np.concatenate([inst([[0, -3, 0]], 1.0), inst([[0, 0, 0]], -1.0), inst([[0, 0, 0]], -2.0), inst([[0, 0, 0]], -1.0)])
    rays = np.concatenate([api.rays([[-0.25, -0.5, -0.25]], [[0, -1, 0]]), api.rays([[-0.25, -0.5, -0.25]], [[0, -1, 0]], t_max=-0.75)])
    return sc, [imodel(0, 1, instances)], rays


def test_negative_scale(ctx):
    """scale < 0 mirrors the origin through the instance: only a ray that starts inside the sphere can hit, and its t is negative - below every
    positive t and ordered among the negative ones as `<` orders them"""
    sc, models, rays = negative_scene()
    rc = caster(ctx, sc)
    im = attach(ctx, rc, sc, models)
    rc.cast(rays)
    want_im, want = expect(rc, sc, rays, "negative scale")
    # (t_model 0.5, 0.25 and 0.5: every product is -0.5, the first of them stays; below t_max = -0.75 there is none)
    assert want_im["is_hit"].tolist() == [1, 0] and want_im["t"][0] == f32(-0.5) and want_im["subindex"][0] == 1 and not want["is_hit"].any()
    sc2, models2, _ = negative_scene(second=True)
    im2 = attach(ctx, rc, sc2, models2)
    rc.cast(rays[:1])
    want_im, _ = expect(rc, sc2, rays[:1], "negative scales, the more negative second")
    assert want_im["subindex"][0] == 1 and want_im["t"][0] == f32(-0.75)
    rc.setInstancedModels(None)


def test_t_max_around_the_hit(ctx):
    sc = no_entities([[mesh(TRI_Y)]])
    models = [imodel(0, 0, inst([[0, 0, 0]], 1.0))]
    t = RIO.cast_im(dict(sc, im_models=[dict(models[0], radius=sc["models"][0]["origin_radius"])]), ydown(0.25, 0.25, y=5.3))["t"][0]
    rays = np.concatenate([ydown(0.25, 0.25, y=5.3, t_max=v) for v in (np.nextafter(t, f32(0)), t, np.nextafter(t, f32(np.inf)), f32(np.inf))])
    want_im, _ = check(ctx, sc, models, rays, "t_max")
    assert t > 5 and want_im["is_hit"].tolist() == [0, 0, 1, 1]


def skipped_scene():
    sc = no_entities([[mesh(TRI_Y)], [mesh(TRI_Y)]], ready=[1, 0])
    models = [imodel(0, 4, inst([[0, 0, 0]])), imodel(-1, 5, inst([[0, -1, 0]])), imodel(1, 6, inst([[0, -1, 0]])), imodel(0, 8, inst([[0, -2, 0]]))]
    rays = np.concatenate([ydown(0.25, 0.25), ydown(0.25, 0.25, ignore=4), ydown(0.25, 0.25, ignore=8), ydown(0.25, 0.25, ignore=5)])
    return sc, models, rays


def test_skipped_models(ctx):
    """ignore == the model's entity; ray_model = -1; a model that is not ready: each lets the model behind it through"""
    want_im, _ = check(ctx, *skipped_scene(), "skipped models")
    assert want_im["entity"].tolist() == [4, 8, 4, 4] and want_im["t"].tolist() == [5, 7, 5, 5]


# ---- ties and edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [1, 64, api.RAY_BLOCK, "model"])
def test_twin_instances_lowest_slot_wins(ctx, second):
    sc = no_entities([[mesh(TRI_Y)]])
    first = 3
    if second == "model":
        models = [imodel(0, 1, inst([[0, 9, 0]] * 5)), imodel(0, 2, inst([[0, 0, 0]] * 2)), imodel(0, 3, inst([[0, 0, 0]] * 2))]
        want_im, _ = check(ctx, sc, models, ydown(0.25, 0.25), "twins across models", twice=True)
        assert (want_im["model"][0], want_im["subindex"][0], want_im["entity"][0]) == (1, 0, 2)
        return
    pos = np.tile(f32([0, 9, 0]), (first + second + 5, 1))  # (above the ray's origin: they never pass the sphere)
    pos[first] = pos[first + second] = 0
    want_im, _ = check(ctx, sc, [imodel(0, 1, inst(pos))], ydown(0.25, 0.25), f"twin at +{second}", twice=True)
    assert want_im["subindex"][0] == first


def hero_places(n):
    edges = [e for e in (64, api.RAY_BLOCK, api.IM_TILE) if e < n]
    return sorted({0, n - 1} | {e - 1 for e in edges} | set(edges))


@pytest.mark.parametrize("sizes", [(1, 63, 64, 65), (255, 256, 257), (api.IM_TILE - 1, api.IM_TILE), (api.IM_TILE + 1,)])
@pytest.mark.parametrize("reverse", [False, True])
def test_model_sizes_and_nearest_places(ctx, sizes, reverse):
    """Per size one model: the instances on its wave / tile / IM_TILE edges stand in a column under the rays, 4 apart, the others above every
    origin. Ray j starts above the j-th of them: the nearest is the first of those it can see (`reverse`: the last), the rest are farther."""
    sc = no_entities([[mesh(TRI_Y)]])
    models, rays, nearest = [], [], []
    for k, n in enumerate(sizes):
        places = hero_places(n)
        pos = np.tile(f32([40 * k, 900, 0]), (n, 1))
        for j, p in enumerate(places):
            pos[p, 1] = -4 * (len(places) - 1 - j if reverse else j)
        models.append(imodel(0, 10 + k, inst(pos)))
        for j, p in enumerate(places):
            rays.append(ydown(40 * k + 0.25, 0.25, y=pos[p, 1] + 2))
            nearest.append((k, p))
    rays = np.concatenate(rays)
    want_im, _ = check(ctx, sc, models, rays, f"sizes {sizes}")
    assert list(zip(want_im["model"].tolist(), want_im["subindex"].tolist())) == nearest and (want_im["t"] == 2).all()


def test_padding_slots_yield_nothing(ctx):
    """a one-instance model ahead of a second one: the slots between them still hold the 300 instances the first model had before"""
    sc = no_entities([[mesh(TRI_Y)]])
    rc = caster(ctx, sc)
    models = [imodel(0, 1, inst([[0, 0, 0]] * 300)), imodel(0, 2, inst([[0, -2, 0]] * 3))]
    im = attach(ctx, rc, sc, models)
    im.setInstances(0, inst([[50, 0, 0]]))
    models[0]["instances"] = im.readInstances(0)
    rays = np.concatenate([ydown(0.25, 0.25), ydown(50.25, 0.25)])
    rc.cast(rays)
    want_im, _ = expect(rc, sc, rays, "padding")
    assert rc.imCounts()["candidates"] == 4 and want_im["model"].tolist() == [1, 0] and want_im["t"].tolist() == [7, 5]
    rc.setInstancedModels(None)


def stacked_y(n, hero):
    """n parallel triangles one under the other, the nearest at ordinal `hero`"""
    tris = np.tile(np.array(TRI_Y, f32) * f32(4) - f32([1, 0, 1]), (n, 1, 1))
    tris[:, :, 1] = -(f32(1) + np.arange(n, dtype=f32)[:, None] * f32(0.001))
    tris[hero, :, 1] = 0
    return tris


def test_shared_and_distinct_ray_models_and_a_large_mesh(ctx):
    """three models share ray-table model 0, two more have their own; model 2's mesh crosses the narrow phase's split (RAY_BLOCK * RAY_RUN + 1
    triangles, the nearest the last one); lod0_from = 2 is added to the mesh index"""
    n = CHUNK + 1
    sc = no_entities([[mesh(TRI_Y)], [cube(0.5)], [mesh(filler(2)), mesh(stacked_y(n, n - 1), np.uint32)]], lod0_from=[0, 0, 2])
    models = [imodel(0, 1, inst([[0, 0, 0], [10, 0, 0]])), imodel(0, 2, inst([[0, -1, 0], [20, 0, 0]]), origin=(0.5, 0, 0)), imodel(0, 3, inst([[10, 1, 0]], 2.0)),
              imodel(1, 4, inst([[30, 0, 0], [30, 2, 0.1]], 1.5, (0.1, 0.2, 0.3))), imodel(2, 5, inst([[40, 0, 0], [40, -3, 0]], 0.5))]
    rays = np.concatenate([ydown(x + 0.25, 0.25) for x in (0, 10, 20.5, 30, 40)] + [ydown(0.6, 0.25, ignore=1)])
    want_im, _ = check(ctx, sc, models, rays, "shared and distinct", twice=True, max_candidates=1 << 12)
    assert want_im["entity"].tolist() == [1, 3, 2, 4, 5, 2] and want_im["mesh"][4] == 3 and want_im["triangle"][4] == n - 1


# ---- the join with the model instances --------------------------------------------------------------------------------------------
def test_combined_nearer_farther_equal(ctx):
    # entities 0..2: TRI_Y at y = 0 under x = 0, 10, 20; instanced copies above (nearer), below (farther) and in the same place (equal t)
    sc = scene_of([[mesh(TRI_Y)]], [0, 0, 0], transforms([[0, 0, 0], [10, 0, 0], [20, 0, 0]]))
    models = [imodel(0, 9, inst([[0, 1, 0], [10, -1, 0], [20, 0, 0]]))]
    rays = np.concatenate([ydown(x + 0.25, 0.25) for x in (0, 10, 20)])
    want_im, want = check(ctx, sc, models, rays, "combined", twice=True)
    assert want_im["is_hit"].tolist() == [1, 1, 1] and want_im["t"].tolist() == [4, 6, 5]
    assert want["is_hit"].tolist() == [0, 1, 0] and want["entity"][1] == 1 and want["t"][1] == 5  # `new_t < hit.t` is strict (:2746)
    assert want[0].tobytes() == bytes(api.RAY_HIT.itemsize)


def test_skinned_model_instance_and_unskinned_instanced_copy(ctx):
    """entity 1 carries a bent pose that moves its triangle away; the instanced copy of the same model is cast in the bind shape (pose = nullptr)"""
    n_bones = 3
    sk, smodel, rel_pos, rel_rot = rig(ctx, n_bones, bent=True)
    tri = np.array(TRI, f32) + f32([(n_bones - 1) * 0.05 + 0.5, -0.25, 0])
    skin = np.concatenate([skin_of(2, n_bones - 1), skin_of(1, n_bones - 1, n_bones - 2, 0.75)])
    smesh = sk.addMesh(tri, skin)
    sk.setInstances([smodel], [smesh])
    sk.uploadPoses(rel_pos, rel_rot)
    sk.setMode(api.SKIN_EXACT)
    sk.run()
    mats = sk.readPalette(0)["columns"]
    posed = RO._skin(tri, skin, mats)
    sc = scene_of([[mesh(tri, skin=skin)]], [-1, 0], transforms([[0, 0, 0], [0, 0, 0]]), palettes={1: mats}, extra_points=posed)
    at = lambda p, dz=0.0: down(p[:, 0].mean(), p[:, 1].mean() + dz)
    rays = np.concatenate([at(tri), at(posed), at(tri, 100.0)])
    models = [imodel(0, 5, inst([[0, 0, -1], [0, 100, 0]]))]
    rc = caster(ctx, sc, skin_of_entity=np.array([-1, 0], np.int32))
    im = attach(ctx, rc, sc, models)
    rc.cast(rays)
    want_im, want = expect(rc, sc, rays, "skinned next to instanced")
    assert want_im["is_hit"].tolist() == [1, 0, 1] and want_im["t"][0] == 6 and want["is_hit"].tolist() == [0, 1, 0] and want["entity"][1] == 1
    rc.setInstancedModels(None)
    sk.setInstances([smodel], [smesh])  # (no palette behind the instance table any more)


def three_models(n_rays=65):
    rng = np.random.default_rng(23)
    sc = scene_of([[cube(0.5)], [mesh(TRI_Y)]], [0] * 6, transforms(rng.uniform(-20, 20, (6, 3)), scale=rng.uniform(1, 3, (6, 3)).astype(f32)))
    models = []
    for k, n in enumerate((300, 70, 129)):
        rot = rng.uniform(-0.5, 0.5, (n, 3)).astype(f32)
        models.append(imodel(k % 2, 20 + k, inst(rng.uniform(-20, 20, (n, 3)), rng.uniform(0.5, 2.5, n).astype(f32), rot), origin=rng.uniform(-3, 3, 3)))
    o = rng.uniform(-30, 30, (n_rays, 3))
    target = np.stack([models[r % 3]["instances"]["pos"][r % 64].astype(np.float64) + models[r % 3]["origin"] for r in range(n_rays)])
    d = target - o
    d /= np.sqrt((d ** 2).sum(1))[:, None]
    rays = api.rays(o, d)
    rays["ignore"][::9] = 21
    rays["t_max"][::5] = rng.uniform(10, 60, len(rays["t_max"][::5])).astype(f32)
    return sc, models, rays


def test_ray_tile_edges_run_twice(ctx):
    sc, models, rays = three_models(api.RAY_BROAD_RAYS + 1)
    want_im, want = check(ctx, sc, models, rays, "65 rays x 3 models", twice=True)
    edge = [0, api.RAY_BROAD_RAYS - 1, api.RAY_BROAD_RAYS]
    assert want_im["is_hit"].sum() > 30 and want_im["is_hit"][edge].sum() + want["is_hit"][edge].sum() >= 2 and len(set(want_im["model"][want_im["is_hit"] == 1])) == 3


def golden_scene():
    """The scene of tests/golden/rays_im_small.npz: 2 models (a cube, a two-mesh model with lod0_from = 1) of 120 + 70 instances at
    (1e6, 50, -1e6), 100 rays with ignore and finite t_max."""
    rng = np.random.default_rng(31)
    base = np.array([1.0e6, 50.0, -1.0e6])
    sc = no_entities([[cube(0.5)], [mesh(TRI_Y), cube(0.25)]], lod0_from=[0, 1])
    models = []
    for k, n in enumerate((120, 70)):
        rot = rng.uniform(-0.55, 0.55, (n, 3)).astype(f32)
        models.append(imodel(k, 40 + k, inst(rng.uniform(-15, 15, (n, 3)), rng.uniform(0.4, 2.5, n).astype(f32), rot), origin=base + rng.uniform(-2, 2, 3)))
    o = base + rng.uniform(-25, 25, (100, 3))
    pick = rng.integers(0, 70, 100)
    target = np.stack([models[r % 2]["instances"]["pos"][pick[r]].astype(np.float64) + models[r % 2]["origin"] for r in range(100)]) + rng.uniform(-0.2, 0.2, (100, 3))
    d = target - o
    rays = api.rays(o, d / np.sqrt((d ** 2).sum(1))[:, None])
    rays["ignore"][::7] = 40
    rays["t_max"][::4] = rng.uniform(5, 40, len(rays["t_max"][::4])).astype(f32)
    return sc, models, rays


def test_golden_fixture(ctx):
    """tests/golden/rays_im_small.npz: one small scene's inputs and the hits of the REFERENCE's own castRayInstancedModels, compiled from the
    reference tree when the fixture was made (tests/golden/make_golden_rays_im.py; tests/test_ray_im_oracle_vs_ref.py)."""
    g = np.load(os.path.join(GOLDEN, "rays_im_small.npz"))
    meshes = [{"positions": g[f"mesh{k}_positions"], "indices": g[f"mesh{k}_indices"], "skin": None} for k in range(int(g["n_meshes"]))]
    sc = {"meshes": meshes, "models": g["models"].view(api.RAY_MODEL).reshape(-1), "inst_model": np.array([-1], np.int32), "inst_flags": np.array([EV], np.uint8),
          "transforms": transforms([[0, 0, 0]]), "palettes": {}}
    models = [imodel(int(g["im_ray_model"][k]), int(g["im_entity"][k]), g[f"im{k}_instances"].view(api.IM_INSTANCE).reshape(-1), g["im_origin"][k]) for k in range(int(g["n_im_models"]))]
    rays = g["rays"].view(api.RAY).reshape(-1)
    want_im, _ = check(ctx, sc, models, rays, "golden")
    for k in ("is_hit", "entity", "subindex", "mesh", "t"):
        assert want_im[k].tobytes() == g["hit_" + k].tobytes(), f"the oracle and the reference's recorded hits differ in {k}"
    assert want_im["is_hit"].sum() > 30


# ---- the rest -----------------------------------------------------------------------------------------------------------------------
def test_overflow_of_the_instanced_stage(ctx):
    sc, models, rays = three_models()
    rc = caster(ctx, sc)
    im = attach(ctx, rc, sc, models)
    need = RIO.candidates_im(sc, rays)
    want_im, want = RIO.cast_all(sc, rays)
    need_entities = RO.candidates(sc, RIO.effective_rays(rays, want_im))
    cap = max(need // 3, need_entities)  # (the entity stage itself fits)
    assert cap < need
    rc.reserve(len(rays), cap)
    rc.cast(rays)
    assert rc.imCounts() == {"rays": len(rays), "candidates": need, "overflow": 1}
    assert rc.counts()["overflow"] & 2
    guard = rc.readCandidates()[cap:]
    assert len(guard) == api.RAYS_GUARD_BYTES // api.RAY_CANDIDATE.itemsize and (guard.view(np.uint8) == 0xA5).all()
    rc.reserve(len(rays), max(need, need_entities))  # exactly what it asked for
    rc.cast(rays)
    expect(rc, sc, rays, "after the larger reserve")
    rc.setInstancedModels(None)


def test_detach_restores_the_plain_cast(ctx):
    sc, rays, _, _ = seeded()
    rays = rays[:70]
    rc = caster(ctx, sc)
    rc.cast(rays)
    plain, plain_counts = rc.readHits().tobytes(), rc.counts()
    assert code(rc.imCounts) == NOT_BUILT and code(rc.readImHits) == NOT_BUILT
    im = attach(ctx, rc, sc, [imodel(0, 900, inst(sc["transforms"]["pos"][:50], 3.0))])
    rc.cast(rays)
    want_im, _ = expect(rc, sc, rays, "attached")
    assert want_im["is_hit"].any() and rc.readHits().tobytes() != plain
    rc.setInstancedModels(None)
    rc.cast(rays)
    assert rc.readHits().tobytes() == plain and rc.counts() == plain_counts and code(rc.imCounts) == NOT_BUILT
    # lmx_im_destroy of the attached object detaches it
    rc.setInstancedModels(im, [0], [900])
    im.close()
    rc.cast(rays)
    assert rc.readHits().tobytes() == plain and code(rc.imCounts) == NOT_BUILT


def test_set_instances_after_attach_is_seen(ctx):
    sc = no_entities([[mesh(TRI_Y)]])
    models = [imodel(0, 1, inst([[0, 0, 0]]))]
    rc = caster(ctx, sc)
    im = attach(ctx, rc, sc, models)
    rays = np.concatenate([ydown(0.25, 0.25), ydown(70.25, 0.25)])
    rc.cast(rays)
    assert expect(rc, sc, rays, "before")[0]["is_hit"].tolist() == [1, 0]
    im.setInstances(0, inst([[70, 900, 0]] * api.IM_TILE + [[70, 1, 0]] * 2))  # (the arrays move: the span grows)
    models[0]["instances"] = im.readInstances(0)
    im.setOrigins([[0, 0.5, 0]])
    models[0]["origin"] = np.array([0, 0.5, 0])
    rc.cast(rays)
    want_im, _ = expect(rc, sc, rays, "after")
    assert want_im["is_hit"].tolist() == [0, 1] and want_im["t"][1] == 3.5
    rc.setInstancedModels(None)


def test_empty_batch_and_device_rays_stay_unmodified(ctx):
    from tests.conftest import hostsim_active

    sc = scene_of([[mesh(TRI_Y)]], [0], transforms([[10, 0, 0]]))
    rc = caster(ctx, sc)
    im = attach(ctx, rc, sc, [imodel(0, 1, inst([[0, 0, 0], [10, 1, 0]]))])
    rc.cast(np.zeros(0, api.RAY))
    assert rc.imCounts() == {"rays": 0, "candidates": 0, "overflow": 0} and len(rc.readImHits()) == 0 and len(rc.readHits()) == 0
    rays = np.concatenate([ydown(0.25, 0.25), ydown(10.25, 0.25), ydown(5.0, 0.25)])
    before = rays.tobytes()
    if hostsim_active():  # the simulated device's memory is the host's
        rc.castDevice(rays.ctypes.data, len(rays))
        expect(rc, sc, np.frombuffer(before, api.RAY), "device rays")
        after = rays.tobytes()
    else:
        import ctypes as C

        path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
        hip = C.CDLL(path)
        d_rays = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_rays), C.c_size_t(rays.nbytes)) == 0
        try:
            assert hip.hipMemcpy(d_rays, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), C.c_int(1)) == 0  # hipMemcpyHostToDevice
            rc.castDevice(d_rays.value, len(rays))
            expect(rc, sc, rays, "device rays")  # (synchronizes)
            back = np.zeros_like(rays)
            assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), d_rays, C.c_size_t(rays.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
            after = back.tobytes()
        finally:
            assert hip.hipFree(d_rays) == 0
    assert after == before, "the cast wrote the caller's rays"
    assert rc.readImHits()["is_hit"].tolist() == [1, 1, 0] and rc.readHits()["is_hit"].tolist() == [0, 0, 0]
    h, c = rc.deviceImOutputs()
    assert h and c
    rc.setInstancedModels(None)
    assert code(rc.deviceImOutputs) == NOT_BUILT


def code(fn, *a):
    with pytest.raises(api.LumixError) as e:
        fn(*a)
    return e.value.code


def test_error_codes():
    c, other = api.Context(0), api.Context(0)
    try:
        rc = api.RayCaster(c)
        m = mesh(TRI_Y)
        rc.addMesh(m["positions"], m["indices"])
        from tests.test_gpu_rays import model_of

        rc.setModels(np.array([model_of([m], 0)], api.RAY_MODEL))
        im, foreign = api.InstancedModels(c), api.InstancedModels(other)
        im.addModel([1e8, -1, -1, -1], [(0, 0), (0, -1), (0, -1), (0, -1), (0, -1)], 1.5, [3])
        foreign.addModel([1e8, -1, -1, -1], [(0, 0), (0, -1), (0, -1), (0, -1), (0, -1)], 1.5, [3])
        assert code(rc.setInstancedModels, im, [1], [0]) == INVALID        # a ray model past the table
        assert code(rc.setInstancedModels, im, [0, 0], [0, 1]) == INVALID  # more models than the object has
        assert code(rc.setInstancedModels, foreign, [0], [0]) == INVALID   # another context's object
        rc.setInstancedModels(im, [-1], [0])
        rc.setInstancedModels(im, [], [])
        rc.setInstancedModels(im, [0], [3])
        assert code(rc.imCounts) == NOT_BUILT and code(rc.readImHits) == NOT_BUILT and code(rc.deviceImOutputs) == NOT_BUILT  # no reserve, no cast
        im.setInstances(0, inst([[0, 0, 0]]))
        rc.setInstances([-1], [EV])
        rc.reserve(2, 16)
        api.DrawCommands(c).setTransforms(transforms([[0, 0, 0]]))
        rc.cast(ydown(0.25, 0.25))
        got = rc.readImHits()
        assert got["is_hit"].tolist() == [1] and got["entity"][0] == 3 and got["t"][0] == 5
        out = np.zeros(1, api.RAY_IM_HIT)
        rc.cast(np.concatenate([ydown(0.25, 0.25)] * 2))
        assert c.lib.lmx_rays_read_im_hits(c.h, out.ctypes.data, 1) == CAPACITY
        im.close()
        foreign.close()
    finally:
        c.close()
        other.close()
