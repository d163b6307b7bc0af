"""The read-out entry points of the host layer (lmx_*_read_*, lmx_*_counts), one small scene per unit, each held to the same four rules:

  * a capacity one short of what the run left is refused with the code the table states, and the caller's array is left as it was;
  * the exact capacity succeeds and gives what a generous capacity gives, nothing behind it is written;
  * a guard reader (pose buffer, light records, light entities, map, ray candidates, particle channels and frame, compressed blocks, chain
    pixels) given the buffer's whole room returns the guard's fill bytes behind the payload, and given more than that leaves what lies
    behind the room alone;
  * a null array with something to read gives the code the table states. The units disagree about that - INVALID_ARGUMENT in the
    instanced models, the grass, the voxels, the probes, the texture compressor and the Animators' exact-size readers, CAPACITY in the
    particles, silently skipped (OK) in draw, clusters, rays, poses, keys, the animation compressor and the optional outputs of the
    Animators - and the table records it. Where a null array is refused, the table also states the code of a null array
    at a capacity one short: CAPACITY where the capacity is checked first, INVALID_ARGUMENT in the texture compressor, which looks at the
    pointer first.

Runs on the MI355X and under `pytest -m gpu --hostsim`."""
import ctypes as C

import numpy as np
import pytest

from lumixengine_amd import api, scenes
from tests import cluster_oracle as CO
from tests import controller_cases as K
from tests import draw_cases as DC
from tests import particle_asm as A

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CAPACITY = 0, 1, 5
FILL, GUARD, PAD = 0x5C, 0xA5, 64  # what the caller's arrays hold before a call; the guards' fill byte; bytes behind every array
SKIP = None  # "null" of an output the table passes no null for
f32 = np.float32


class Reader:
    """One read-out: call(cap, *pointers) -> code. `used`: what the run left, in the units of cap; dtypes / counts(cap): the element type
    and count of every output array; short: the code of cap = used - 1; null[i]: the code of a null output i at a generous cap;
    exact: the entry point takes the count itself, not a capacity (anything else is `short`). A guard reader has room (the buffer with its
    guard, in the units of cap) and guard, the [first, end) element ranges of output 0 that hold the fill byte. null_short, where given: the
    code of a null output 0 at cap = used - 1, which pins the order of the two refusals."""

    def __init__(self, call, dtypes, used, null, counts=None, short=CAPACITY, exact=False, room=None, guard=(), null_short=None):
        self.call, self.dtypes, self.used, self.null, self.short, self.exact = call, [np.dtype(d) for d in dtypes], int(used), null, short, exact
        self.counts = counts or (lambda cap: (cap,) * len(dtypes))
        self.room, self.guard, self.null_short = room, guard, null_short

    def run(self, cap, null=None):
        """-> (code, the outputs' bytes with PAD bytes behind each)"""
        bufs = [np.full(n * d.itemsize + PAD, FILL, np.uint8) for n, d in zip(self.counts(cap), self.dtypes)]
        ptrs = [None if i == null else b.ctypes.data_as(C.c_void_p) for i, b in enumerate(bufs)]
        return self.call(cap, *ptrs), bufs


def check(r: Reader, name):
    sizes = lambda cap: [n * d.itemsize for n, d in zip(r.counts(cap), r.dtypes)]
    generous = r.used if r.exact else (r.used if r.room is None else r.room) + 5
    rc, want = r.run(generous)
    assert rc == OK, f"{name}: a generous capacity gives {rc}"
    holds = sizes(r.used if r.room is None else r.room)  # bytes the entry point may write
    for w, h in zip(want, holds):
        assert (w[h:] == FILL).all(), f"{name}: written behind what it holds"
    if r.used:
        rc, got = r.run(r.used - 1)
        assert rc == r.short, f"{name}: cap = used - 1 = {r.used - 1} gives {rc}"
        assert all((g == FILL).all() for g in got), f"{name}: a refused call wrote to the caller's array"
    rc, got = r.run(r.used)
    assert rc == OK, f"{name}: cap = used = {r.used} gives {rc}"
    for g, w, n in zip(got, want, sizes(r.used)):
        assert g[:n].tobytes() == w[:n].tobytes(), f"{name}: cap = used differs from the generous read"
        assert (g[n:] == FILL).all(), f"{name}: cap = used wrote behind the array"
    if r.room is not None:
        rc, got = r.run(r.room)
        assert rc == OK, name
        item = r.dtypes[0].itemsize
        assert r.guard and all(b > a for a, b in r.guard)
        for a, b in r.guard:
            assert (got[0][a * item : b * item] == GUARD).all(), f"{name}: the guard [{a}, {b}) does not hold its fill bytes"
            assert (want[0][a * item : b * item] == GUARD).all(), name
        assert (got[0][r.room * item :] == FILL).all(), name
    for i, code in enumerate(r.null):
        if code is SKIP:
            continue
        rc, got = r.run(generous, null=i)
        assert rc == code, f"{name}: a null output {i} gives {rc}, the table says {code}"
    if r.null_short is not None:
        assert r.used, name
        rc, got = r.run(r.used - 1, null=0)
        assert rc == r.null_short, f"{name}: a null output at cap = used - 1 gives {rc}, the table says {r.null_short}"
        assert all((g == FILL).all() for g in got), f"{name}: a refused call wrote to the caller's array"


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
KEEP = []  # the wrappers and objects of every scene: alive until the module's contexts close


def u32():
    return C.c_uint32(0)


def draw_scene(ctx, R, N):
    """four sorted pairs and the hand-made instancer CSR"""
    from tests.test_gpu_draw_commands import upload_tables

    sc, dt, lod, tr = DC.tables()
    sk, dc = upload_tables(ctx, sc, dt, tr, DC.N_ENTITIES)
    keys, values, n_batches, _ = DC.arrays("a pair type the key run never emits")
    assert len(keys) == 4
    dc.runPairs(DC.view(), keys, values, n_batches, *DC.instancer())
    c = dc.counts()
    assert c["runs"] and c["instance_bytes"] and c["group_records"]
    lib, h = ctx.lib, ctx.h
    R["draw_read_runs"] = Reader(lambda cap, p: lib.lmx_draw_read_runs(h, p, cap), [api.DRAW_RUN], c["runs"], [OK])
    R["draw_read_instance_data"] = Reader(lambda cap, p: lib.lmx_draw_read_instance_data(h, p, cap), [np.uint8], c["instance_bytes"], [OK])
    R["draw_read_group_data"] = Reader(lambda cap, p: lib.lmx_draw_read_group_data(h, p, cap), [np.uint8], c["group_records"] * 48, [OK])
    N["draw_counts"] = (lambda p: lib.lmx_draw_counts(h, p), api.DRAW_COUNTS, INVALID_ARGUMENT)


def keys_scene(ctx, R, N):
    """sixty entities, six of them skinned, culled and keyed"""
    from tests.test_gpu_pose_processor import chain_scene

    base, sc, dt, tr, table, skinned = chain_scene(n_mesh=60, n_skinned=6, seed=71)
    n = len(table)
    cs = api.CullingSystem(ctx)
    cs.build(base["entity"], np.zeros(n, np.uint8), tr["pos"], base["radius"])
    sk = api.SortKeys(ctx)
    sk.setModels(sc["models"], sc["mesh_types"])
    sk.setInstances(sc["model"], sc["material_offset"], sc["mesh_materials"], sc["lod"], sc["flags"], sc["dirty"], sc["pose_frame"])
    sk.setPositions(tr["pos"])
    cam = (0.0, 0.0, 420.0)
    cs.cull(api.viewport_frustum(pos=cam, far=1000.0))
    sk.run(api.keys_view(camera_pos=cam, time_delta=1 / 60, frame_number=7, layer_to_bucket=sc["layer_to_bucket"], bucket_depth_sorted=sc["bucket_depth_sorted"]), 15)
    KEEP.append((cs, sk))
    c = sk.counts()
    assert c["pairs"] and c["poses"] and not c["overflow"], c
    lib, h = ctx.lib, ctx.h
    offsets = np.zeros(15 + 2, np.uint32)
    KEEP.append(offsets)
    R["keys_read_pairs"] = Reader(lambda cap, k, v: lib.lmx_keys_read_pairs(h, k, v, cap), [np.uint64, np.uint64], c["pairs"], [OK, OK])
    R["keys_read_instancer"] = Reader(lambda cap, v: lib.lmx_keys_read_instancer(h, api._ptr(offsets), v, cap), [np.uint64], c["instanced"], [OK])
    R["keys_read_poses"] = Reader(lambda cap, p: lib.lmx_keys_read_poses(h, p, cap), [np.int32], c["poses"], [OK])
    R["keys_read_dirty"] = Reader(lambda cap, p: lib.lmx_keys_read_dirty(h, p, cap), [np.int32], c["dirty"], [OK])
    R["keys_read_state"] = Reader(lambda cap, lod, fr: lib.lmx_keys_read_state(h, lod, fr, cap), [np.float32, np.uint32], n, [OK, OK], short=INVALID_ARGUMENT, exact=True)
    N["keys_counts"] = (lambda p: lib.lmx_keys_counts(h, p), api.KEYS_COUNTS, INVALID_ARGUMENT)


def clusters_scene(ctx, R, N):
    """eight lights and one probe of each kind on 2 x 1 x 16 clusters"""
    from tests.test_gpu_clusters import filler

    sc = CO.scene()
    env_on, refl_on = (np.flatnonzero(sc[k]["flags"] & api.PROBE_ENABLED)[:1] for k in ("env", "refl"))
    probes = {"env": sc["env"][env_on], "env_entities": sc["env_entities"][env_on], "refl": sc["refl"][refl_on], "refl_entities": sc["refl_entities"][refl_on]}
    max_lights, map_capacity = 16, 512
    cf = filler(ctx, sc["transforms"], sc["lights"], sc["atlas"], probes, max_lights, map_capacity)
    cf.runList(CO.view(128, 64), np.arange(8, dtype=np.int32))
    c = cf.counts()
    assert c["lights"] == 8 and c["env_probes"] == 1 and c["refl_probes"] == 1 and 0 < c["map_entries"] <= map_capacity and not c["overflow"], c
    lib, h = ctx.lib, ctx.h
    g_rec, g_word = api.CLUSTERS_GUARD_BYTES // 64, api.CLUSTERS_GUARD_BYTES // 4
    R["clusters_read_lights"] = Reader(lambda cap, p: lib.lmx_clusters_read_lights(h, p, cap), [api.CLUSTER_LIGHT], 8, [OK], room=max_lights + g_rec,
                                       guard=[(max_lights, max_lights + g_rec)])
    R["clusters_read_light_entities"] = Reader(lambda cap, p: lib.lmx_clusters_read_light_entities(h, p, cap), [np.int32], 8, [OK], room=max_lights + g_word,
                                               guard=[(max_lights, max_lights + g_word)])
    R["clusters_read_map"] = Reader(lambda cap, p: lib.lmx_clusters_read_map(h, p, cap), [np.int32], c["map_entries"], [OK], room=map_capacity + g_word,
                                    guard=[(map_capacity, map_capacity + g_word)])
    R["clusters_read_clusters"] = Reader(lambda cap, p: lib.lmx_clusters_read_clusters(h, p, cap, None), [api.CLUSTER], 2 * 1 * 16, [OK])
    R["clusters_read_probes.env"] = Reader(lambda cap, p: lib.lmx_clusters_read_probes(h, p, cap, None, 0), [api.CLUSTER_ENV_PROBE], 1, [OK])
    R["clusters_read_probes.refl"] = Reader(lambda cap, p: lib.lmx_clusters_read_probes(h, None, 0, p, cap), [api.CLUSTER_REFL_PROBE], 1, [OK])
    N["clusters_counts"] = (lambda p: lib.lmx_clusters_counts(h, p), api.CLUSTERS_COUNTS, INVALID_ARGUMENT)


def poses_scene(ctx, R, N):
    """one skinned instance of two bones, listed once"""
    sk = api.Skinning(ctx)
    sk.setMode(True)
    sk.setPoseWriteback(True)
    s = scenes.skeleton(2, seed=3)
    model = sk.addModel(s["parents"], s["bind"], s["first_nonroot"])
    mesh_id = sk.addMesh(*scenes.skinned_mesh(8, 2, seed=4))
    sk.setInstances([model], [mesh_id])
    pos, rot = scenes.relative_poses(1, 2, seed=5)
    sk.uploadPoses(pos.reshape(-1, 3), rot.reshape(-1, 4))
    sk.run()
    pp = api.PoseProcessor(ctx)
    pp.setInstances([-1, 0, -1])
    pp.beginFrame(7, 0)
    pp.runList([1])
    c = pp.counts()
    assert c == {"instances": 1, "bytes": 64, "skipped": 0, "overflow": 0}, c
    lib, h = ctx.lib, ctx.h
    reserved = 2 * 32  # every instance's bones once
    R["poses_read_buffer"] = Reader(lambda cap, p: lib.lmx_poses_read_buffer(h, p, cap), [np.uint8], c["bytes"], [OK], room=reserved + api.POSES_GUARD_BYTES,
                                    guard=[(reserved, reserved + api.POSES_GUARD_BYTES)])
    R["poses_read_slices"] = Reader(lambda cap, a, b: lib.lmx_poses_read_slices(h, a, b, cap), [np.uint32, np.uint32], 3, [OK, OK])
    N["poses_counts"] = (lambda p: lib.lmx_poses_counts(h, p), api.POSES_COUNTS, INVALID_ARGUMENT)


def rays_scene(ctx, R, N):
    """two rays against one triangle model, an instanced copy of it, one procedural triangle and one flat terrain"""
    from tests.test_gpu_rays import TRI, caster, down, mesh, scene_of, transforms
    from tests.test_gpu_rays_im import attach, imodel, inst
    from tests.test_gpu_rays_scene import geom, terrain

    sc = scene_of([[mesh(TRI)]], [0] + [-1] * 7, transforms(np.zeros((8, 3))))
    max_rays, max_cand = 4, 8
    rc = caster(ctx, sc, max_rays=max_rays, max_candidates=max_cand)
    im = attach(ctx, rc, sc, [imodel(0, 7, inst([[3, 0, 0]]))])
    rc.setProceduralGeometries([geom(1, np.asarray(TRI, f32) + f32([0, 0, -2]))])
    rc.setTerrains([terrain(2, np.zeros((4, 4), np.uint16))])
    rc.cast(np.concatenate([down(0.25, 0.25), down(0.6, 0.6)]))
    KEEP.append((rc, im))
    assert rc.counts()["rays"] == 2 and rc.imCounts()["rays"] == 2 and rc.sceneCounts()["rays"] == 2
    lib, h = ctx.lib, ctx.h
    g = api.RAYS_GUARD_BYTES // api.RAY_CANDIDATE.itemsize
    R["rays_read_hits"] = Reader(lambda cap, p: lib.lmx_rays_read_hits(h, p, cap), [api.RAY_HIT], 2, [OK])
    R["rays_read_candidates"] = Reader(lambda cap, p: lib.lmx_rays_read_candidates(h, p, cap), [api.RAY_CANDIDATE], 0, [OK], room=max_cand + g, guard=[(max_cand, max_cand + g)])
    R["rays_read_im_hits"] = Reader(lambda cap, p: lib.lmx_rays_read_im_hits(h, p, cap), [api.RAY_IM_HIT], 2, [OK])
    R["rays_read_pg_hits"] = Reader(lambda cap, p: lib.lmx_rays_read_pg_hits(h, p, cap), [api.RAY_PG_HIT], 2, [OK])
    R["rays_read_terrain_hits"] = Reader(lambda cap, p: lib.lmx_rays_read_terrain_hits(h, p, cap), [api.RAY_TERRAIN_HIT], 2 * 1, [OK])
    R["rays_read_scene_hits"] = Reader(lambda cap, p: lib.lmx_rays_read_scene_hits(h, p, cap), [api.RAY_SCENE_HIT], 2, [OK])
    N["rays_counts"] = (lambda p: lib.lmx_rays_counts(h, p), api.RAYS_COUNTS, INVALID_ARGUMENT)
    N["rays_im_counts"] = (lambda p: lib.lmx_rays_im_counts(h, p), api.RAYS_IM_COUNTS, INVALID_ARGUMENT)
    N["rays_scene_counts"] = (lambda p: lib.lmx_rays_scene_counts(h, p), api.RAYS_SCENE_COUNTS, INVALID_ARGUMENT)


def im_scene(ctx, R, N):
    """one instanced model of five instances in front of the camera"""
    im = api.InstancedModels(ctx)
    m = im.addModel([1e8, -1, -1, -1], [(0, 0), (0, -1), (0, -1), (0, -1), (0, -1)], 1.0, [3])
    inst = np.zeros(5, api.IM_INSTANCE)
    inst["pos"][:, 0], inst["pos"][:, 2], inst["scale"] = np.arange(5) - 2.0, -10.0, 1.0
    im.setInstances(m, inst)
    fr = api.frustum_perspective((0, 0, 0), np.array([0, 0, -1], f32), np.array([0, 1, 0], f32), float(np.deg2rad(70)), 16 / 9, 0.1, 300.0)
    im.run(api.im_view(camera_pos=(0, 0, 0)), fr)
    KEEP.append(im)
    total = int(im.counts()["bin_count"].sum())
    assert total == 5 and len(im.readIndirect()) == 1
    lib, h = ctx.lib, im.h
    R["im_read_instances"] = Reader(lambda cap, p: lib.lmx_im_read_instances(h, m, p, cap), [api.IM_INSTANCE], 5, [INVALID_ARGUMENT])
    R["im_counts"] = Reader(lambda cap, p: lib.lmx_im_counts(h, 0, p, cap), [api.IM_COUNTS], 1, [INVALID_ARGUMENT], null_short=CAPACITY)
    R["im_read_records"] = Reader(lambda cap, p: lib.lmx_im_read_records(h, 0, p, cap, C.byref(u32())), [api.IM_INSTANCE], total, [INVALID_ARGUMENT], null_short=CAPACITY)
    R["im_read_indirect"] = Reader(lambda cap, p: lib.lmx_im_read_indirect(h, 0, p, cap, C.byref(u32())), [api.IM_INDIRECT], 1, [INVALID_ARGUMENT], null_short=CAPACITY)
    N["im_read_grid"] = (lambda p: lib.lmx_im_read_grid(h, m, p), api.IM_GRID, INVALID_ARGUMENT)


def grass_scene(ctx, R, N):
    """one quad in one slot, seen by one view"""
    from tests.test_gpu_grass import EVERYTHING, device, full_splat, heightmap, one_quad_type, terrain, view

    ty, centre = one_quad_type(0.5, 1, 2)
    g = device(ctx, [terrain("all", heightmap(64, 64), full_splat(64, 64), [ty])], 1)
    g.update(5, [centre])
    g.cull([view(EVERYTHING, (centre[0], 10.0, centre[1]))])  # (inside the type's distance of the quad)
    KEEP.append(g)
    c = g.counts()
    assert len(g.readQuads()) == 1 and c[0]["draws"] == 1, c
    lib, h = ctx.lib, g.h
    S = api.GRASS_SLOT_INSTANCES
    R["grass_read_quads"] = Reader(lambda cap, p: lib.lmx_grass_read_quads(h, p, cap, C.byref(u32())), [api.GRASS_QUAD], 1, [INVALID_ARGUMENT])
    R["grass_read_instances"] = Reader(lambda cap, p: lib.lmx_grass_read_instances(h, 0, p, cap), [api.GRASS_INSTANCE], S, [INVALID_ARGUMENT], null_short=CAPACITY)
    R["grass_read_draws"] = Reader(lambda cap, p: lib.lmx_grass_read_draws(h, 0, p, cap, C.byref(u32())), [api.GRASS_DRAW], 1, [INVALID_ARGUMENT], null_short=CAPACITY)
    R["grass_counts"] = Reader(lambda cap, p: lib.lmx_grass_counts(h, p, cap), [api.GRASS_COUNTS], 1, [INVALID_ARGUMENT], null_short=CAPACITY)


def particles_scene(ctx, R, N):
    """one emitter of capacity 8 holding five particles, stepped and filled once"""
    from tests.particle_asm import CH, LIT, OUT, SYS

    emit = [A.mov(CH(0), SYS(A.EMIT_INDEX)), A.mov(CH(1), LIT(0.0)), A.mov(CH(2), LIT(3.0))]
    p = A.Program([A.add(CH(1), CH(1), SYS(A.TIME_DELTA))], emit, [A.mov(OUT(0), CH(0)), A.mul(OUT(1), CH(1), LIT(2.0))], channels=3, registers=2, outputs=2, init_emit_count=5)
    ps = api.ParticleSystems(ctx)
    ps.addSystem(1, 0)
    p.set_on(ps, 0, 0)
    ps.reserve(0, 0, 8)
    ps.setSeed(0)
    ps.update(0.25)
    ps.fill()
    KEEP.append(ps)
    assert int(ps.counts()[0]["particles"]) == 5
    lib, h = ctx.lib, ps.h
    cap8, stride, G = 8, 8 + api.PARTICLES_GUARD_FLOATS, api.PARTICLES_GUARD_FLOATS
    frame_bytes = ps.deviceOutputs().frame_bytes
    assert frame_bytes == 8 * 2 * 4
    one_slice = np.zeros(1, api.PARTICLE_SLICE)
    KEEP.append(one_slice)
    R["particles_counts"] = Reader(lambda cap, p: lib.lmx_particles_counts(h, p, cap), [api.PARTICLES_COUNTS], 1, [CAPACITY])
    # a channel's guard lies behind the channel: the buffer's room is what the run holds
    R["particles_read_channels"] = Reader(lambda cap, p: lib.lmx_particles_read_channels(h, 0, 0, p, cap, C.byref(u32())), [np.float32], 3 * stride, [CAPACITY], room=3 * stride,
                                          guard=[(c * stride + cap8, (c + 1) * stride) for c in range(3)])
    R["particles_read_slices.slices"] = Reader(lambda cap, p: lib.lmx_particles_read_slices(h, p, cap, None, 0), [api.PARTICLE_SLICE], 1, [CAPACITY])
    R["particles_read_slices.frame"] = Reader(lambda cap, p: lib.lmx_particles_read_slices(h, api._ptr(one_slice), 1, p, cap), [np.uint8], frame_bytes + 4 * G, [OK],
                                              room=frame_bytes + 4 * G, guard=[(frame_bytes, frame_bytes + 4 * G)])


def animators_scene(ctx, R, N):
    """one Animator of the first controller case, updated once"""
    from tests.test_gpu_animators import input_values, setup

    sk, an, world, ids, ctl, w = setup(ctx, [0], with_world=False)
    sk.setAnimables([ids[0]], [0])
    an.setInputs(0, 1, input_values([0], 0))
    an.update(K.CASES[0]["frames"][0][0])
    KEEP.append((sk, an))
    first, instrs = an.readInstrs()
    state = an.readState(0)
    n_bones = len(K.SKELETONS[K.CASES[0]["model"]]["parents"])
    assert len(instrs) and len(state)
    lib, h = ctx.lib, ctx.h
    first_out = np.zeros(2, np.uint32)
    KEEP.append(first_out)
    R["animators_read_root_motion"] = Reader(lambda cap, p: lib.lmx_animators_read_root_motion(h, p, cap), [api.LOCAL_RIGID], 1, [INVALID_ARGUMENT], short=INVALID_ARGUMENT, exact=True)
    R["animators_read_state"] = Reader(lambda cap, p: lib.lmx_animators_read_state(h, 0, p, cap, C.byref(u32())), [np.uint8], len(state), [OK])
    R["animators_read_instrs"] = Reader(lambda cap, p: lib.lmx_animators_read_instrs(h, api._ptr(first_out), 1, p, cap, C.byref(u32())), [api.BLEND_INSTR], len(instrs), [OK])
    R["anim_read_times"] = Reader(lambda cap, p: lib.lmx_anim_read_times(h, p, cap), [np.uint32], 1, [INVALID_ARGUMENT], short=INVALID_ARGUMENT, exact=True)
    R["anim_read_pose"] = Reader(lambda cap, pos, rot: lib.lmx_anim_read_pose(h, 0, pos, rot, cap), [np.float32, np.float32], n_bones, [OK, OK], counts=lambda cap: (3 * cap, 4 * cap))


def voxels_scene(ctx, R, N):
    """one triangle in a grid of max_res 2, four rays of AO per cell"""
    vx = api.Voxels(ctx)
    vx.voxelize([(f32([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]]), np.array([0, 1, 2], np.uint16))], 2)
    vx.computeAO(4, 1, 2)
    KEEP.append(vx)
    cells = vx._cells()
    assert 1 < cells <= 128 and vx.read().any(), cells
    lib, h = ctx.lib, vx.h
    R["voxels_read"] = Reader(lambda cap, p: lib.lmx_voxels_read(h, p, cap), [np.uint8], cells, [INVALID_ARGUMENT], null_short=CAPACITY)
    R["voxels_read_ao"] = Reader(lambda cap, p: lib.lmx_voxels_read_ao(h, p, cap), [np.float32], cells, [INVALID_ARGUMENT], null_short=CAPACITY)
    N["voxels_info"] = (lambda p: lib.lmx_voxels_info(h, p), api.VOXELS_INFO, INVALID_ARGUMENT)


def probes_scene(ctx, R, N):
    """one cubemap of size 16 (the smallest a mip run takes): its SH, its mips, its radiance levels and their RGBM bytes"""
    pb = api.ProbeBaker(ctx)
    pb.setCubemaps(np.random.default_rng(16).random((1, 6, 16, 16, 4), dtype=f32))
    pb.shRun()
    pb.filterRun()
    KEEP.append(pb)
    lib, h = ctx.lib, pb.h
    mips, levels = 4 * api.probe_mip_texels(16), 4 * pb._level_texels()  # floats of the mips; floats of the levels = their RGBM bytes
    rows = dict(null=[INVALID_ARGUMENT], null_short=CAPACITY)
    R["probes_read_sh"] = Reader(lambda cap, p: lib.lmx_probes_read_sh(h, p, cap), [np.float32], 1, counts=lambda cap: (27 * cap,), **rows)  # (cap in probes)
    R["probes_read_mips"] = Reader(lambda cap, p: lib.lmx_probes_read_mips(h, p, cap), [np.float32], mips, **rows)
    R["probes_read_filtered"] = Reader(lambda cap, p: lib.lmx_probes_read_filtered(h, p, cap), [np.float32], levels, **rows)
    R["probes_read_rgbm"] = Reader(lambda cap, p: lib.lmx_probes_read_rgbm(h, p, cap), [np.uint8], levels, **rows)


def texcomp_scene(ctx, R, N):
    """one 4 x 4 image as one BC1 block; one 4 x 4 chain and its two generated levels"""
    px = np.random.default_rng(4).integers(0, 256, (1, 4, 4, 4), dtype=np.uint8)
    blocks, chain = api.TexCompressor(ctx), api.TexCompressor(ctx)
    blocks.setImages([px[0]])
    blocks.run(api.TEX_BC1)
    chain.setChains(px)
    chain.generateMips(api.TEXMIP_LINEAR)
    KEEP.append((blocks, chain))
    lib, G = ctx.lib, api.TEXCOMP_GUARD_BYTES
    n_blocks, n_pixels = api.TEX_BLOCK_BYTES[api.TEX_BC1], api.texcomp_chain_bytes(1, 4, 4)
    assert n_blocks == 8 and n_pixels == 4 * (16 + 4 + 1)
    # both refuse a null array first, then a short one; both hold a guard behind what they read
    R["texcomp_read"] = Reader(lambda cap, p: lib.lmx_texcomp_read(blocks.h, p, cap), [np.uint8], n_blocks, [INVALID_ARGUMENT], room=n_blocks + G, guard=[(n_blocks, n_blocks + G)],
                               null_short=INVALID_ARGUMENT)
    R["texcomp_read_pixels"] = Reader(lambda cap, p: lib.lmx_texcomp_read_pixels(chain.h, p, cap), [np.uint8], n_pixels, [INVALID_ARGUMENT], room=n_pixels + G,
                                      guard=[(n_pixels, n_pixels + G)], null_short=INVALID_ARGUMENT)


def animcomp_scene(ctx, R, N):
    """one clip of two bones and two samples, every track of it animated"""
    from tests import animcomp_cases as AC

    k = np.zeros((2, 2, 7), f32)
    k[0, :, 3:] = [0, 0, 0, 1]
    k[1, :, 3:] = [0.6, 0, 0, 0.8]
    k[1, :, :3] = [[5, 0, 0], [0, -7, 3]]
    ac = api.AnimCompressor(ctx)
    ac.setClips([AC.clip("two bones, two samples", k, np.zeros((2, 3), f32))])
    ac.run()
    KEEP.append(ac)
    info = ac.clipInfo(0)
    assert info["status"] == 0 and info["translation_stream_size"] and info["rotation_stream_size"], info
    most = max(info[f] for f in ("n_const_translations", "n_translations", "n_const_rotations", "n_rotations"))
    used = {"tracks": most, "translation_stream": info["translation_stream_size"], "rotation_stream": info["rotation_stream_size"]}
    lib, h = ctx.lib, ac.h
    tables = [api.ANIM_CONST_TRANSLATION, api.ANIM_TRANSLATION_TRACK, api.ANIM_CONST_ROTATION, api.ANIM_ROTATION_TRACK]

    def row(which):
        """the capacity `which` is the reader's cap, the other two are generous; every array has the room its own capacity states, or more"""
        def call(cap, *arrays):
            caps = {f: n + 5 for f, n in used.items()}
            caps[which] = cap
            out = api.LmxAnimCompOutput(*arrays, caps["tracks"], 0, caps["translation_stream"], caps["rotation_stream"])
            return lib.lmx_animcomp_read_clip(h, 0, C.byref(out))

        def counts(cap):
            n = dict(used)
            n[which] = cap
            return (n["tracks"],) * 4 + (n["translation_stream"], n["rotation_stream"])

        return Reader(call, tables + [np.uint8, np.uint8], used[which], [OK] * 6, counts=counts, null_short=CAPACITY)

    for which in used:
        R["animcomp_read_clip." + which] = row(which)
    N["animcomp_clip_info"] = (lambda p: lib.lmx_animcomp_clip_info(h, 0, p), np.dtype((np.uint8, C.sizeof(api.LmxAnimCompInfo))), INVALID_ARGUMENT)


SCENES = {"draw": draw_scene, "keys": keys_scene, "clusters": clusters_scene, "poses": poses_scene, "rays": rays_scene, "im": im_scene, "grass": grass_scene,
          "particles": particles_scene, "animators": animators_scene, "voxels": voxels_scene, "probes": probes_scene, "texcomp": texcomp_scene,
          "animcomp": animcomp_scene}
READERS = {
    "draw": ["draw_read_runs", "draw_read_instance_data", "draw_read_group_data"],
    "keys": ["keys_read_pairs", "keys_read_instancer", "keys_read_poses", "keys_read_dirty", "keys_read_state"],
    "clusters": ["clusters_read_lights", "clusters_read_light_entities", "clusters_read_map", "clusters_read_clusters", "clusters_read_probes.env", "clusters_read_probes.refl"],
    "poses": ["poses_read_buffer", "poses_read_slices"],
    "rays": ["rays_read_hits", "rays_read_candidates", "rays_read_im_hits", "rays_read_pg_hits", "rays_read_terrain_hits", "rays_read_scene_hits"],
    "im": ["im_read_instances", "im_counts", "im_read_records", "im_read_indirect"],
    "grass": ["grass_read_quads", "grass_read_instances", "grass_read_draws", "grass_counts"],
    "particles": ["particles_counts", "particles_read_channels", "particles_read_slices.slices", "particles_read_slices.frame"],
    "animators": ["animators_read_root_motion", "animators_read_state", "animators_read_instrs", "anim_read_times", "anim_read_pose"],
    "voxels": ["voxels_read", "voxels_read_ao"],
    "probes": ["probes_read_sh", "probes_read_mips", "probes_read_filtered", "probes_read_rgbm"],
    "texcomp": ["texcomp_read", "texcomp_read_pixels"],
    "animcomp": ["animcomp_read_clip.tracks", "animcomp_read_clip.translation_stream", "animcomp_read_clip.rotation_stream"],
}
# the readers of fixed size: a record the caller always has room for, so only the null rule applies
NULL_ONLY = {"draw": ["draw_counts"], "keys": ["keys_counts"], "clusters": ["clusters_counts"], "poses": ["poses_counts"],
             "rays": ["rays_counts", "rays_im_counts", "rays_scene_counts"], "im": ["im_read_grid"], "grass": [], "particles": [], "animators": [], "voxels": ["voxels_info"], "probes": [],
             "texcomp": [], "animcomp": ["animcomp_clip_info"]}


@pytest.fixture(scope="module")
def built():
    """unit -> (readers, fixed-size readers), every scene on a context of its own: the units share the draw pass's transform source and the
    pose tables, and a scene must not change what another one's run left"""
    out, ctxs = {}, []
    try:
        for unit, make in SCENES.items():
            ctx = api.Context(0)
            ctxs.append(ctx)
            R, N = {}, {}
            make(ctx, R, N)
            assert sorted(R) == sorted(READERS[unit]) and sorted(N) == sorted(NULL_ONLY[unit]), unit
            out[unit] = (R, N)
        yield out
    finally:
        while KEEP:  # (the objects before their contexts: their destructors read them)
            k = KEEP.pop()
            for o in k if isinstance(k, tuple) else (k,):
                if hasattr(o, "close"):
                    o.close()
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("unit,name", [(u, n) for u, names in READERS.items() for n in names])
def test_read_out(built, unit, name):
    check(built[unit][0][name], name)


@pytest.mark.parametrize("unit,name", [(u, n) for u, names in NULL_ONLY.items() for n in names])
def test_fixed_size_read_out(built, unit, name):
    call, dtype, null_code = built[unit][1][name]
    out = np.full(np.dtype(dtype).itemsize + PAD, FILL, np.uint8)
    assert call(out.ctypes.data_as(C.c_void_p)) == OK, name
    assert (out[np.dtype(dtype).itemsize :] == FILL).all(), name
    assert call(None) == null_code, name
