"""Voxels on the device (lmx_voxels_*, voxel_kernels.hip) against tests/voxel_oracle.py and the reference's recorded outputs
(tests/golden/voxels_small.npz): voxel bytes, AO float bit patterns, the generator's state, lookups and baked u8 values, all exact.

Also passes on the simulated device: pytest -m gpu tests/test_gpu_voxels.py --hostsim (the option last: it takes an optional value).

Shapes (voxel_oracle.cases()): a unit cube at max_res 4 (7^3) with 64 and 65 rays - one chunk of 64 lanes, then a voxel's rays across
two chunks, the second call continuing the first one's stream; a 3:2:1 slab at 9 (three different strides, 32-bit indices, 5 rays:
twelve voxels share a chunk); a flat quad (the thin axis has resolution 3) with 1 and 32 rays; a sphere of 2 000 triangles at 13 (16^3
cells: sixteen waves, four blocks of k_voxel_ao); two meshes with 16- and 32-bit indices, strides of 20 and 28 bytes and unreferenced
vertices outside the AABB; a caller's box smaller than the mesh with a triangle larger than the grid (its cell box is split over several
waves of k_voxel_raster) and two zero-area triangles; the two constructed seeds on an occupied bottom layer. The global-memory form of
k_voxel_ao takes grids over 327 680 cells; test_global_form runs it on a 70 x 70 x 70 grid with one ray per voxel."""
import os

import numpy as np
import pytest

from tests import voxel_oracle as VO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxels_small.npz")
_expected = {}


def expected(name):
    """the oracle's outputs of a case, computed once and shared (read-only)"""
    if name not in _expected:
        r = VO.run_case(VO.cases()[name])
        for v in r.values():
            v.setflags(write=False)
        _expected[name] = r
    return _expected[name]


def bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    if a.tobytes() != b.tobytes():
        view = np.uint8 if a.itemsize == 1 else np.uint32
        bad = np.nonzero(a.reshape(-1).view(view) != b.reshape(-1).view(view))[0]
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at {bad[:5]}: {a.reshape(-1)[bad[:5]]} vs {b.reshape(-1)[bad[:5]]}")


def build(api, ctx, c):
    v = api.Voxels(ctx)
    if c["begin"] is None:
        v.voxelize(c["meshes"], c["max_res"])
    else:
        v.beginRaster(c["begin"][0], c["begin"][1], c["max_res"])
        for p, i in c["meshes"]:
            v.raster(p, i)
    return v


def device_case(api, ctx, c, points, verts):
    """the pipeline of voxel_oracle.run_case through the C ABI"""
    v = build(api, ctx, c)
    info = v.info()
    r = dict(aabb_min=info["aabb_min"].copy(), aabb_max=info["aabb_max"].copy(), voxel_size=np.array([info["voxel_size"]], np.float32), resolution=info["resolution"].copy(),
             voxels=v.read())
    u, w = c["seed"]
    for k, rc in enumerate(c["ao"]):
        v.computeAO(rc, u, w)
        u, w = v.rngState()
        r[f"ao{k}"] = v.readAO()
        r[f"rng{k}"] = np.array([u, w], np.uint32)
    r["points"] = points
    r["sample"], r["sample_inside"] = v.sample(points)
    r["sample_ao"], inside = v.sampleAO(points)
    assert inside.tobytes() == r["sample_inside"].tobytes()
    r["bake_vertices"] = verts
    r["bake_raw_0"] = v.bakeVertexAO(verts, 0.0)
    r["bake_raw_03"] = v.bakeVertexAO(verts, 0.3)
    v.blurAO()
    r["blurred"] = v.readAO()
    r["bake_0"] = v.bakeVertexAO(verts, 0.0)
    r["bake_03"] = v.bakeVertexAO(verts, 0.3)
    v.close()
    return r


@pytest.mark.parametrize("name", list(VO.cases()))
def test_case_matches_oracle_and_reference(gpu_ctx, name):
    from lumixengine_amd import api

    c = VO.cases()[name]
    want = expected(name)
    got = device_case(api, gpu_ctx, c, want["points"], want["bake_vertices"])
    g = np.load(GOLDEN)
    for k in want:
        bits(got[k], want[k], f"{name}: {k} against the oracle")
        bits(got[k], g[f"{name}|{k}"], f"{name}: {k} against the reference's record")
    assert want["sample_inside"].min() == 0 and want["sample_inside"].max() == 1
    inside = want["bake_raw_0"] != 0xEE  # (no AO of these cases bakes to the fill byte)
    assert want["bake_raw_03"].max() == 255 and (want["bake_raw_0"][inside] < 255).any() and (want["bake_raw_0"] != want["bake_raw_03"]).any()


def test_two_raster_calls_equal_one(gpu_ctx):
    from lumixengine_amd import api

    p, i = VO.sphere_mesh(8, 10, 1.0, (0, 0, 0))
    mn, mx = p.min(axis=0), p.max(axis=0)
    one, two = api.Voxels(gpu_ctx), api.Voxels(gpu_ctx)
    one.beginRaster(mn, mx, 9)
    one.raster(p, i)
    two.beginRaster(mn, mx, 9)
    half = len(i) // 6 * 3
    two.raster(p, i[:half])
    first = two.read()
    two.raster(p, i[half:].astype(np.uint16))
    o = VO.Voxels()
    o.beginRaster(mn, mx, 9)
    o.raster(p, i[:half])
    bits(first, o.voxels, "the first half")
    o.raster(p, i[half:])
    bits(two.read(), o.voxels, "both halves")
    bits(one.read(), two.read(), "one call against two")
    assert 0 < first.sum() < o.voxels.sum()
    one.close()
    two.close()


def test_set_copies_grid_voxels_and_ao(gpu_ctx):
    from lumixengine_amd import api

    c = VO.cases()["slab"]
    want = expected("slab")
    src, dst = build(api, gpu_ctx, c), api.Voxels(gpu_ctx)
    dst.beginRaster((0, 0, 0), (1, 1, 1), 3)  # (another grid, replaced by the copy)
    src.computeAO(c["ao"][0], *c["seed"])
    dst.set(src)
    src.beginRaster((0, 0, 0), (1, 1, 1), 3)  # the source changes; the copy keeps what it was given
    bits(dst.info()["resolution"], want["resolution"], "resolution")
    bits(dst.read(), want["voxels"], "voxels")
    bits(dst.readAO(), want["ao0"], "AO")
    dst.blurAO()
    bits(dst.readAO(), want["blurred"], "blurred")
    empty = api.Voxels(gpu_ctx)
    with pytest.raises(api.LumixError) as e:
        dst.set(empty)
    assert e.value.code == 6
    for v in (src, dst, empty):
        v.close()


def test_ray_counts_and_stream_continuation(gpu_ctx):
    """ray_count 1, 5, 32, 64, 65 on one grid, each call continuing the stream the one before it left"""
    from lumixengine_amd import api

    c = VO.cases()["cube"]
    v = build(api, gpu_ctx, c)
    o = VO.Voxels()
    o.voxelize(c["meshes"], c["max_res"])
    u, w = 2463534242, 88172645
    for rc in (1, 5, 32, 64, 65):
        v.computeAO(rc, u, w)
        o.computeAO(rc, u, w)
        bits(v.readAO(), o.ao, f"AO with {rc} rays")
        assert v.rngState() == o.rng, rc
        assert v.rngState() == api.voxels_rng_skip(u, w, 3 * rc * len(o.voxels))
        u, w = v.rngState()
    v.close()


def test_global_form(gpu_ctx):
    """a grid of 70^3 = 343 000 cells is over what k_voxel_ao stages in LDS: the march reads the bytes in global memory"""
    from lumixengine_amd import api

    p, i = VO.box_mesh((0, 0, 0), (1, 1, 1))
    v, o = api.Voxels(gpu_ctx), VO.Voxels()
    v.voxelize([(p, i)], 67)
    o.voxelize([(p, i)], 67)
    assert len(o.voxels) > 32 * api.VOXEL_AO_LDS_WORDS
    bits(v.info()["resolution"], o.res.astype(np.int32), "resolution")
    bits(v.read(), o.voxels, "voxels")
    v.computeAO(1, 13, 57)
    o.computeAO(1, 13, 57)
    bits(v.readAO(), o.ao, "AO")
    assert v.rngState() == o.rng
    assert 0.0 < o.ao.mean() < 1.0
    v.close()


def test_both_forms_of_the_ao_kernel_agree(gpu_ctx):
    """LMX_VOXELS_OPT_AO_LDS = 0 marches a small grid through global memory: the same AO as the LDS form and the oracle"""
    from lumixengine_amd import api

    c = VO.cases()["two meshes"]
    want = expected("two meshes")
    v = build(api, gpu_ctx, c)
    for lds in (0, 1):
        v.setOption(api.VOXELS_OPT_AO_LDS, lds)
        v.computeAO(c["ao"][0], *c["seed"])
        bits(v.readAO(), want["ao0"], f"AO with LMX_VOXELS_OPT_AO_LDS = {lds}")
    with pytest.raises(api.LumixError) as e:
        v.setOption(7, 1)
    assert e.value.code == 1
    v.close()


def test_refusals(gpu_ctx):
    from lumixengine_amd import api

    INVALID, NOT_BUILT = 1, 6
    p, i = VO.box_mesh((0, 0, 0), (1, 1, 1))

    def refused(code, fn, *args):
        with pytest.raises(api.LumixError) as e:
            fn(*args)
        assert e.value.code == code, e.value

    v = api.Voxels(gpu_ctx)
    refused(NOT_BUILT, v.raster, p, i)
    refused(NOT_BUILT, v.computeAO, 4, 1, 1)
    refused(NOT_BUILT, v.read)
    refused(NOT_BUILT, v.sample, np.zeros((1, 3), np.float32))
    refused(INVALID, v.beginRaster, (0, 0, 0), (1, 1, 1), 0)
    refused(INVALID, v.beginRaster, (0, 0, 0), (1, np.inf, 1), 4)
    refused(INVALID, v.beginRaster, (0, 0, 0), (0, 0, 0), 4)
    refused(INVALID, v.beginRaster, (0, 0, 0), (1, 1, 1), 2000)  # 2003^3 cells
    bad = p.copy()
    bad[3, 1] = np.nan
    refused(INVALID, v.voxelize, [(bad, i)], 4)
    refused(INVALID, v.voxelize, [(p, (i + 3).astype(np.uint16))], 4)  # an index past n_vertices
    refused(INVALID, v.voxelize, [(p, i[:4])], 4)
    v.voxelize([(p, i)], 4)
    refused(INVALID, v.raster, p, (i + 3).astype(np.uint16))
    refused(INVALID, v.computeAO, 0, 1, 1)
    refused(INVALID, v.computeAO, 4, 0, 1)
    refused(NOT_BUILT, v.blurAO)
    refused(NOT_BUILT, v.readAO)
    refused(NOT_BUILT, v.rngState)
    refused(NOT_BUILT, v.sampleAO, np.zeros((1, 3), np.float32))
    refused(NOT_BUILT, v.bakeVertexAO, p, 0.0)
    v.computeAO(4, 1, 1)
    v.blurAO()
    v.beginRaster((0, 0, 0), (1, 1, 1), 4)  # a new grid drops the AO
    refused(NOT_BUILT, v.blurAO)
    d = v.deviceOutputs()
    assert d.d_voxels and not d.d_ao and d.n_cells == 343
    v.close()
