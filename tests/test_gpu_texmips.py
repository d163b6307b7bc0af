"""Mip chains on the device (lmx_texcomp_set_chains / generate_mips / read_pixels, texmips_kernels.hip) against tests/texmips_oracle.py and
the reference's recorded levels (tests/golden/texmips_small.npz). Whole chains are bit for bit the oracle's in all three modes, with
coverage scaling on and off; per level, from the recorded previous level, the filtered modes are within 1 of the recorded stb bytes and
under the caps of DESIGN.md §4.24 (at most 0.1 % of the bytes differ in linear mode, 2 % in sRGB mode).

Also passes on the simulated device: pytest -m gpu tests/test_gpu_texmips.py --hostsim (the option last: it takes an optional value).

Shapes, the smallest that reach each path (k_mip_tail makes every level behind the first whose sides are both at most 32): 1 x 1 (no level
to make); 8 x 8, 3 x 3, 8 x 1 and 1 x 8 (the tail alone, from level 0; a copied axis); 32 x 32 (the largest level the tail starts from) and
33 x 32 (one texel more: one level launch, then the tail); 37 x 21 (one level launch, then 9 -> 4, 5 -> 2 and 2 -> 1 on different axes in
the tail); 128 x 64 (level launches over several tiles, the width crossing 32 a level after the height, then the tail); 64 x 16 (the tail
starts at 32 x 8); 34 x 8 and 8 x 34 (one output texel beyond a 16 x 16 tile along x, along y); batches of 1 and 7."""
import os

import numpy as np
import pytest

from tests import texcomp_oracle as TO
from tests import texmips_oracle as MO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texmips_small.npz")
INVALID, CAPACITY, NOT_BUILT = 1, 5, 6
MODES = (MO.LINEAR, MO.SRGB, MO.STOCHASTIC)
LINEAR_CAP, SRGB_CAP = 0.001, 0.02
SHAPES = ((1, 1, 1), (8, 8, 1), (8, 1, 1), (1, 8, 1), (37, 21, 7), (3, 3, 1), (128, 64, 1), (34, 8, 1), (8, 34, 1), (32, 32, 1), (33, 32, 7), (64, 16, 1))  # (w, h, batch)
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(GOLDEN))
    return _cache["g"]


def images_of(w, h, n):
    rng = np.random.default_rng(w * 131 + h * 7 + n)
    img = rng.integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    img[:, : h // 2, : (w + 1) // 2, 3] = 0  # a block of zero alpha: the premultiplied channels decide its neighbours' colour
    return img


def want_of(w, h, n, mode, ref_norm):
    """the oracle's chains, computed once per case and shared (read-only)"""
    key = (w, h, n, mode, ref_norm)
    if key not in _cache:
        v = MO.flatten(MO.chains(images_of(w, h, n), mode, ref_norm))
        v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} vs {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} bytes differ, first (chain, byte) {bad[:5].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def refused(api, code, fn, *args):
    with pytest.raises(api.LumixError) as e:
        fn(*args)
    assert e.value.code == code, e.value


@pytest.mark.parametrize("ref_norm", [-1.0, 0.5])
@pytest.mark.parametrize("mode", MODES)
def test_whole_chains_bit_for_bit(gpu_ctx, mode, ref_norm):
    from lumixengine_amd import api

    tc = api.TexCompressor(gpu_ctx)
    for w, h, n in SHAPES:
        tc.setChains(images_of(w, h, n))
        tc.generateMips(mode, ref_norm)
        got = tc.readPixels()
        assert got.shape == (n, api.texcomp_chain_bytes(n, w, h) // n)
        same(got, want_of(w, h, n, mode, ref_norm), f"{n} chains of {w} x {h}, mode {mode}, coverage {ref_norm}")
        same(api.texmips_host(images_of(w, h, n), mode, ref_norm), got, "the host's arithmetic")
    tc.close()


@pytest.mark.parametrize("mode,cap", [(MO.LINEAR, LINEAR_CAP), (MO.SRGB, SRGB_CAP)])
def test_levels_within_1_of_the_recorded_stb_bytes(gpu_ctx, mode, cap):
    """every recorded level from the recorded level before it, the three fixture images as one batch"""
    from lumixengine_amd import api

    g = golden()
    tc = api.TexCompressor(gpu_ctx)
    compared = differ = 0
    for key, w, h in (("37x21", 37, 21), ("64x48", 64, 48), ("40x24", 40, 24)):
        rec = [api.texcomp_split_chain(c, w, h) for c in g[f"{key}_{'linear' if mode == MO.LINEAR else 'srgb'}"]]
        for m in range(1, len(rec[0])):
            prev = np.stack([chain[m - 1] for chain in rec])
            pw, ph = prev.shape[2], prev.shape[1]
            tc.setChains(prev)
            tc.generateMips(mode)
            got = tc.readPixels()
            for chain, mine in zip(rec, got):
                level = api.texcomp_split_chain(mine, pw, ph)[1]
                d = np.abs(level.astype(int) - chain[m].astype(int))
                assert d.max() <= 1, f"{key} level {m}: a byte differs from stb's by {d.max()}"
                compared, differ = compared + d.size, differ + int((d != 0).sum())
    print(f"\nmode {mode}: {differ} of {compared} bytes differ from the recorded stb bytes ({100.0 * differ / compared:.4f} %)")
    assert [compared, differ] == g[f"share_{'linear' if mode == MO.LINEAR else 'srgb'}"].tolist(), "the device differs where the oracle does, as recorded"
    assert differ <= cap * compared
    tc.close()


def test_stochastic_and_coverage_equal_the_references_record(gpu_ctx):
    """the modes that are the reference's bit for bit: whole recorded chains, the coverage of image 0 for every image"""
    from lumixengine_amd import api

    g = golden()
    tc = api.TexCompressor(gpu_ctx)
    for key in ("37x21", "64x48", "40x24"):
        images = g[f"{key}_images"]
        tc.setChains(images)
        tc.generateMips(MO.STOCHASTIC)
        same(tc.readPixels(), g[f"{key}_stochastic"], f"{key} stochastic")
        tc.generateMips(MO.STOCHASTIC, 0.5)  # (again on the same level-0 images)
        same(tc.readPixels(), g[f"{key}_stochastic_cov"], f"{key} stochastic with coverage scaling")
        assert MO.compute_coverage(images[0], 0.5).tobytes() == g[f"{key}_coverage"].tobytes()
    tc.close()


def coverage_cases():
    rng = np.random.default_rng(21)
    noise = rng.integers(0, 256, (2, 21, 37, 4)).astype(np.uint8)
    opaque_then_holes = noise.copy()
    opaque_then_holes[0, :, :, 3] = 255          # image 0 sets the coverage: 1, so count = 0 ...
    opaque_then_holes[1, :10, :, 3] = 0          # ... and image 1's levels have texels in bin 0: new_ref = 0, an infinite scale, 0 stays 0
    return [("a break inside the walk", noise, 0.5), ("coverage 0: the walk ends at 255", noise, 1.0), ("new_ref 0", opaque_then_holes, 0.5), ("ref 0", noise, 0.0),
            ("ref 0 and new_ref 0: 0 / 0", opaque_then_holes, 0.0), ("ref 1", opaque_then_holes, 1.0)]


@pytest.mark.parametrize("mode", [MO.SRGB, MO.STOCHASTIC])
def test_coverage_edge_cases(gpu_ctx, mode):
    from lumixengine_amd import api

    tc = api.TexCompressor(gpu_ctx)
    for what, images, ref_norm in coverage_cases():
        chains = MO.chains(images, mode, ref_norm)
        if what == "coverage 0: the walk ends at 255":
            assert MO.compute_coverage(images[0], ref_norm) == 0
        if what == "new_ref 0":
            with np.errstate(all="ignore"):
                assert np.isinf(MO.coverage_scale(MO.compute_mip(images[1], 18, 10, mode), ref_norm, np.float32(1.0)))
            assert set(np.unique(chains[1][1][:, :, 3]).tolist()) == {0, 255}, "zero alpha stays 0, everything else goes to 255"
        tc.setChains(images)
        tc.generateMips(mode, ref_norm)
        same(tc.readPixels(), MO.flatten(chains), what)
    tc.close()


def test_device_input_gives_the_same_bytes(gpu_ctx):
    from lumixengine_amd import api

    images = images_of(37, 21, 7)
    up, dev = api.TexCompressor(gpu_ctx), api.TexCompressor(gpu_ctx)
    up.setImages(list(images))  # the first compressor's copy serves as the device buffer: seven images tightly packed
    dev.setChainsDevice(7, 37, 21, up.deviceOutputs().d_rgba)
    dev.generateMips(MO.SRGB, 0.5)
    same(dev.readPixels(), want_of(37, 21, 7, MO.SRGB, 0.5), "chains from device pixels")
    refused(api, INVALID, dev.setChainsDevice, 7, 37, 21, up.deviceOutputs().d_rgba + 2)
    dev.close()
    up.close()


@pytest.mark.parametrize("fmt", [TO.BC1, TO.BC3, TO.BC5])
def test_chain_to_blocks_is_the_payload(gpu_ctx, fmt):
    """set_chains -> generate_mips -> run: the blocks of the oracle's chain, images in (image, mip) order"""
    from lumixengine_amd import api

    w, h, n = 8, 8, 2
    chains = MO.chains(images_of(w, h, n), MO.LINEAR, 0.5)
    blocks = np.concatenate([TO.image_blocks(level) for chain in chains for level in chain])
    assert len(blocks) == n * (4 + 1 + 1 + 1)
    if fmt == TO.BC5:
        want = np.concatenate([TO.encode_bc4(blocks[:, :, 0]), TO.encode_bc4(blocks[:, :, 1])], 1)
    else:
        (o4, _), (o3, _) = TO.encode_bc1_pair(blocks)
        want = o3 if fmt == TO.BC1 else np.concatenate([TO.encode_bc4(blocks[:, :, 3]), o4], 1)
    tc = api.TexCompressor(gpu_ctx)
    tc.setChains(images_of(w, h, n))
    refused(api, NOT_BUILT, tc.run, fmt)  # levels 1 .. are not made yet
    tc.generateMips(MO.LINEAR, 0.5)
    tc.run(fmt)
    got = tc.read()
    assert np.array_equal(got, want), f"format {fmt}: {(got != want).any(1).sum()} of {len(want)} blocks differ"
    d = tc.deviceOutputs()
    assert d.n_images == n * 4 and d.n_blocks == len(blocks) and d.format == fmt
    tc.generateMips(MO.LINEAR)  # other pixels: the blocks of the run before are dropped
    refused(api, NOT_BUILT, tc.read)
    tc.close()


def test_refusals(gpu_ctx):
    from lumixengine_amd import api

    tc = api.TexCompressor(gpu_ctx)
    lib, im = tc.lib, np.zeros((1, 4, 4, 4), np.uint8)
    opt = api.LmxTexMipOptions(MO.LINEAR, -1.0)
    out = np.zeros(1024, np.uint8)
    assert lib.lmx_texcomp_generate_mips(tc.h, api.C.byref(opt)) == NOT_BUILT, "generate_mips without set_chains"
    assert lib.lmx_texcomp_read_pixels(tc.h, out.ctypes.data, out.size) == NOT_BUILT
    tc.setImages([im[0]])
    assert lib.lmx_texcomp_generate_mips(tc.h, api.C.byref(opt)) == NOT_BUILT, "a plain batch is no chain"
    for n, w, h in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.lmx_texcomp_set_chains(tc.h, n, w, h, im.ctypes.data) == INVALID
    assert lib.lmx_texcomp_set_chains(tc.h, 1, 4, 4, None) == INVALID and lib.lmx_texcomp_set_chains_device(tc.h, 1, 4, 4, None) == INVALID
    assert lib.lmx_texcomp_set_chains(None, 1, 4, 4, im.ctypes.data) == INVALID
    assert lib.lmx_texcomp_set_chains_device(tc.h, 1, 16384, 16384, im.ctypes.data) == CAPACITY, "level 0 alone fills LMX_TEXCOMP_MAX_BATCH_BYTES"
    assert lib.lmx_texcomp_set_chains_device(tc.h, 65536, 2, 1, im.ctypes.data) == CAPACITY
    tc.run(TO.BC4)  # a refused set leaves the batch before as it was
    tc.setChains(im)
    assert lib.lmx_texcomp_read_pixels(tc.h, out.ctypes.data, out.size) == NOT_BUILT, "read_pixels before generate_mips"
    assert lib.lmx_texcomp_generate_mips(tc.h, None) == INVALID
    for mode in (-1, 3):
        bad = api.LmxTexMipOptions(mode, -1.0)
        assert lib.lmx_texcomp_generate_mips(tc.h, api.C.byref(bad)) == INVALID
    tc.generateMips(MO.LINEAR)
    need = api.texcomp_chain_bytes(1, 4, 4)
    assert need == 4 * (16 + 4 + 1)
    assert lib.lmx_texcomp_read_pixels(tc.h, out.ctypes.data, need - 1) == CAPACITY and lib.lmx_texcomp_read_pixels(tc.h, None, need) == INVALID
    tc.setImages([im[0]])  # a plain set drops the chains
    assert lib.lmx_texcomp_read_pixels(tc.h, out.ctypes.data, out.size) == NOT_BUILT
    tc.close()


def test_stochastic_refuses_a_side_above_4096(gpu_ctx):
    from lumixengine_amd import api

    tc = api.TexCompressor(gpu_ctx)
    tc.setChains(np.zeros((1, 1, 4097, 4), np.uint8))
    refused(api, CAPACITY, tc.generateMips, MO.STOCHASTIC)
    tc.generateMips(MO.LINEAR)  # the filtered modes take it
    assert not tc.readPixels().any()
    tc.setChains(np.full((1, 1, 4096, 4), 7, np.uint8))
    tc.generateMips(MO.STOCHASTIC)
    assert (tc.readPixels() == 7).all()
    tc.close()


@pytest.mark.parametrize("mode", MODES)
def test_guard_behind_the_chains_stays_untouched(gpu_ctx, mode):
    from lumixengine_amd import api

    tc = api.TexCompressor(gpu_ctx)
    for w, h, n in ((37, 21, 7), (34, 8, 1)):  # the smaller batch in the same buffer: its guard lies inside the larger one's chains
        tc.setChains(images_of(w, h, n))
        tc.generateMips(mode, 0.5)
        px = tc.readPixels()
        raw = tc.readPixels(guard=True)
        assert len(raw) == px.size + api.TEXCOMP_GUARD_BYTES and np.array_equal(raw[: px.size], px.reshape(-1))
        assert (raw[px.size:] == 0xA5).all(), "a kernel wrote behind the last chain"
    tc.close()
