"""The texture compressor on the device (lmx_texcomp_*, texcomp_kernels.hip) against tests/texcomp_oracle.py and the reference's recorded
outputs (tests/golden/texcomp_small.npz). Every bound is exact: byte equality with the oracle, integer equality of the per-block error with
the reference's exhaustive mode, <= against its level 10.

Also passes on the simulated device: pytest -m gpu tests/test_gpu_texcomp.py --hostsim (the option last: it takes an optional value).

Shapes: the fixture's blocks as one image of 42 x 46 blocks; one 4 x 4 image; 4 x 8 and 8 x 4 (block order); 1 x 1, 2 x 2 and 6 x 2 (texels
outside the image); batches of 1 and of 7 images of different sizes whose 21 blocks are no multiple of the four a workgroup takes per round;
and one block more than the largest grid takes in one round (lmx_texcomp_blocks_per_round: 4096, 1024 workgroups of four waves), so that
the first wave comes round a second time - most of the blocks solid, every 61st, the first and the last two noise."""
import os

import numpy as np
import pytest

from tests import texcomp_oracle as TO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texcomp_small.npz")
INVALID, CAPACITY, NOT_BUILT = 1, 5, 6
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(GOLDEN))
    return _cache["g"]


def oracle(key, blocks):
    """the oracle's blocks without and with 3-colour blocks, computed once per key and shared (read-only)"""
    if key not in _cache:
        (o4, e4), (o3, e3) = TO.encode_bc1_pair(blocks)
        for v in (o4, e4, o3, e3):
            v.setflags(write=False)
        _cache[key] = (o4, e4, o3, e3)
    return _cache[key]


def expected(blocks, fmt, key):
    blocks = np.asarray(blocks, np.uint8)
    if fmt == TO.BC4:
        return TO.encode_bc4(blocks[:, :, 0])
    if fmt == TO.BC5:
        return np.concatenate([TO.encode_bc4(blocks[:, :, 0]), TO.encode_bc4(blocks[:, :, 1])], 1)
    o4, _, o3, _ = oracle(key, blocks)
    return o3 if fmt == TO.BC1 else np.concatenate([TO.encode_bc4(blocks[:, :, 3]), o4], 1)


def as_image(blocks, bw):
    """blocks (n, 16, 4), n a multiple of bw -> the image whose row-major blocks they are"""
    n = len(blocks)
    return np.ascontiguousarray(blocks.reshape(n // bw, bw, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(n // bw * 4, bw * 4, 4))


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} blocks differ, first {bad[:5]}: {got[bad[:2]].tolist()} vs {want[bad[:2]].tolist()}"


def refused(api, code, fn, *args):
    with pytest.raises(api.LumixError) as e:
        fn(*args)
    assert e.value.code == code, e.value


def shape_images():
    rng = np.random.default_rng(5)
    sizes = [(4, 4), (4, 8), (8, 4), (1, 1), (2, 2), (6, 2), (13, 9)]  # (w, h): 1 + 2 + 2 + 1 + 1 + 2 + 12 = 21 blocks
    return [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for w, h in sizes]


@pytest.mark.parametrize("fmt", [TO.BC1, TO.BC3, TO.BC4, TO.BC5])
def test_fixture_blocks_match_oracle_and_reference(gpu_ctx, fmt):
    from lumixengine_amd import api

    g = golden()
    blocks = g["rgba"]
    assert len(blocks) == 42 * 46 and np.array_equal(TO.image_blocks(as_image(blocks, 42)), blocks)
    tc = api.TexCompressor(gpu_ctx)
    tc.setImages([as_image(blocks, 42)])
    tc.run(fmt)
    got = tc.read()
    same(got, expected(blocks, fmt, "fixture"), f"format {fmt} against the oracle")
    if fmt == TO.BC1:
        err = TO.block_error(blocks, got)
        assert np.array_equal(err, g["ex_3_err"]), "the per-block error is the exhaustive mode's"
        assert (err <= g["l10_3_err"]).all() and (err < g["l10_3_err"]).any()
        assert TO.decode_bc1(got)[1].any(), "the fixture has blocks that come out 3-colour"
    elif fmt == TO.BC3:
        err = TO.block_error(blocks, got[:, 8:])
        assert np.array_equal(err, g["ex_4_err"]) and (err <= g["l10_4_err"]).all() and (err < g["l10_4_err"]).any()
        assert not TO.decode_bc1(got[:, 8:])[1].any(), "every BC3 block has color0 > color1"
        same(got[:, :8], TO.encode_bc4(blocks[:, :, 3]), "the alpha half")
    elif fmt == TO.BC4:
        same(got, g["bc4"], "BC4 against the reference's record")
    else:
        same(got, g["bc5"], "BC5 against the reference's record")
    d = tc.deviceOutputs()
    assert d.d_blocks and d.d_rgba and d.n_images == 1 and d.n_blocks == len(blocks) and d.format == fmt and d.bytes == got.size
    tc.close()


@pytest.mark.parametrize("fmt", [TO.BC1, TO.BC3, TO.BC5])
def test_shapes_single_images_and_batches(gpu_ctx, fmt):
    """every image alone (n = 1), then all seven as one batch, on one compressor"""
    from lumixengine_amd import api

    images = shape_images()
    per = [TO.image_blocks(im) for im in images]
    assert [len(p) for p in per] == [1, 2, 2, 1, 1, 2, 12] and sum(len(p) for p in per) % 4 != 0
    assert (per[3][0, 1:] == 0).all() and (per[5][:, [2, 3, 6, 7]][1] == 0).all() and (per[5][0, 8:] == 0).all(), "texels outside the image are 0, 0, 0, 0"
    want = expected(np.concatenate(per), fmt, "shapes")
    tc = api.TexCompressor(gpu_ctx)
    at = 0
    for im, p in zip(images, per):
        tc.setImages([im])
        tc.run(fmt)
        same(tc.read(), want[at: at + len(p)], f"a {im.shape[1]} x {im.shape[0]} image alone")
        at += len(p)
    tc.setImages(images)  # n = 7, 21 blocks: images one behind the other in input order
    assert api.texcomp_output_bytes([(im.shape[1], im.shape[0]) for im in images], fmt) == want.size
    tc.run(fmt)
    same(tc.read(), want, "the batch of seven")
    tc.close()


def test_one_more_block_than_a_grid_round(gpu_ctx):
    from lumixengine_amd import api

    grid_round = api.texcomp_blocks_per_round()  # from the library: tests/test_texcomp_cpu.py holds it to the documented 4096
    n = grid_round + 1
    rng = np.random.default_rng(9)
    blocks = np.broadcast_to(rng.integers(0, 256, (n, 1, 4)), (n, 16, 4)).astype(np.uint8)  # solid, a colour per block
    noisy = np.unique(np.concatenate([np.arange(0, n, 61), [grid_round - 1, grid_round]]))
    blocks[noisy] = rng.integers(0, 256, (len(noisy), 16, 4))
    assert n == 17 * 241, "the image below is 241 blocks wide"
    tc = api.TexCompressor(gpu_ctx)
    tc.setImages([as_image(blocks, 241)])
    for fmt in (TO.BC1, TO.BC3):
        tc.run(fmt)
        same(tc.read(), expected(blocks, fmt, "grid round"), f"format {fmt}: {n} blocks")
    tc.close()


def test_device_input_gives_the_same_bytes(gpu_ctx):
    from lumixengine_amd import api

    images = shape_images()
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    up, dev = api.TexCompressor(gpu_ctx), api.TexCompressor(gpu_ctx)
    up.setImages(images)
    dev.setImagesDevice(sizes, up.deviceOutputs().d_rgba)  # the first compressor's copy serves as the device buffer
    for fmt in (TO.BC1, TO.BC5):
        up.run(fmt)
        dev.run(fmt)
        same(dev.read(), up.read(), f"format {fmt}")
    assert dev.deviceOutputs().d_rgba == up.deviceOutputs().d_rgba, "the pixels are not copied"
    dev.close()
    up.close()


def test_probes_to_bc3_payload(gpu_ctx):
    """two 16 x 16 cubemaps: set_cubemaps -> filter_run -> set_from_probes -> run(BC3), no read between; the blocks equal the oracle's on
    lmx_probes_read_rgbm's bytes, per probe face-major, level-minor"""
    from lumixengine_amd import api

    rng = np.random.default_rng(3)
    cubes = (rng.random((2, 6, 16, 16, 4)) ** 3 * 6).astype(np.float32)
    pb, tc = api.ProbeBaker(gpu_ctx), api.TexCompressor(gpu_ctx)
    refused(api, NOT_BUILT, tc.setFromProbes, pb)
    pb.setCubemaps(cubes)
    refused(api, NOT_BUILT, tc.setFromProbes, pb)
    pb.filterRun()
    tc.setFromProbes(pb)
    tc.run(TO.BC3)
    got = tc.read()
    rgbm = pb.readRGBM()
    blocks = np.concatenate([TO.image_blocks(rgbm[p][f][k]) for p in range(2) for f in range(6) for k in range(api.PROBE_LEVELS)])
    assert len(blocks) == 2 * 6 * (16 + 4 + 1 + 1 + 1) and len(got) == len(blocks)
    same(got, expected(blocks, TO.BC3, "probes"), "the probes' .lbc payload")
    assert tc.deviceOutputs().d_rgba == pb.deviceOutputs().d_rgbm
    tc.close()
    pb.close()


def test_refusals(gpu_ctx):
    from lumixengine_amd import api

    tc = api.TexCompressor(gpu_ctx)
    lib, im = tc.lib, np.zeros((4, 4, 4), np.uint8)
    refused(api, NOT_BUILT, tc.run, TO.BC1)
    refused(api, NOT_BUILT, tc.read)
    refused(api, NOT_BUILT, tc.deviceOutputs)
    refused(api, INVALID, tc.setImages, [])
    refused(api, INVALID, tc.setImages, [np.zeros((0, 4, 4), np.uint8)])
    refused(api, INVALID, tc.setImages, [im, np.zeros((4, 0, 4), np.uint8)])
    d = np.array([[4, 4]], np.uint32)
    assert lib.lmx_texcomp_set_images(tc.h, 1, None, im.ctypes.data) == INVALID and lib.lmx_texcomp_set_images(tc.h, 1, d.ctypes.data, None) == INVALID
    assert lib.lmx_texcomp_set_images_device(tc.h, 1, d.ctypes.data, None) == INVALID and lib.lmx_texcomp_set_from_probes(tc.h, None) == INVALID
    big = np.array([[16384, 16385]], np.uint32)  # 4 x 16384 x 16385 bytes: above the cap of 2^30
    assert lib.lmx_texcomp_set_images_device(tc.h, 1, big.ctypes.data, im.ctypes.data) == CAPACITY
    tc.setImages([im])
    refused(api, NOT_BUILT, tc.read)  # a read before a run
    refused(api, INVALID, tc.run, 4)
    refused(api, INVALID, tc.run, -1)
    tc.run(TO.BC3)
    out = np.zeros(16, np.uint8)
    assert lib.lmx_texcomp_read(tc.h, out.ctypes.data, 15) == CAPACITY and lib.lmx_texcomp_read(tc.h, None, 16) == INVALID
    assert lib.lmx_texcomp_device_outputs(tc.h, None) == INVALID
    assert lib.lmx_texcomp_set_images_device(tc.h, 1, d.ctypes.data, tc.deviceOutputs().d_rgba + 1) == INVALID, "device pixels are read as words"
    tc.setImages([im])  # a set drops the blocks of the batch before
    refused(api, NOT_BUILT, tc.read)
    tc.close()


@pytest.mark.parametrize("fmt", [TO.BC1, TO.BC3, TO.BC4, TO.BC5])
def test_guard_behind_the_blocks_stays_untouched(gpu_ctx, fmt):
    from lumixengine_amd import api

    images = shape_images()
    tc = api.TexCompressor(gpu_ctx)
    tc.setImages(images)
    tc.run(fmt)
    blocks = tc.read()
    raw = tc.read(guard=True)
    assert len(raw) == blocks.size + api.TEXCOMP_GUARD_BYTES and np.array_equal(raw[: blocks.size], blocks.reshape(-1))
    assert (raw[blocks.size:] == 0xA5).all(), "a kernel wrote behind the last block"
    tc.setImages(images[:2])  # a smaller batch in the same buffer: its guard lies inside the larger one's blocks
    tc.run(fmt)
    small = tc.read()
    raw = tc.read(guard=True)
    assert (raw[small.size:] == 0xA5).all() and np.array_equal(raw[: small.size].reshape(small.shape), blocks[: len(small)])
    tc.close()
