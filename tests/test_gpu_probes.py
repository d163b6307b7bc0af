"""The probe bake on the device (lmx_probes_*, probe_kernels.hip) against tests/probe_oracle.py and the recorded outputs of the reference
(tests/golden/probes_small.npz): SH coefficients, mip texels, sampler results and RGBM bytes exact; the radiance levels within their bound.

Also passes on the simulated device: pytest -m gpu tests/test_gpu_probes.py --hostsim (the option last: it takes an optional value).

Shapes (probe_oracle.cases()): SH at S = 1, 2, 5, 16, at S = 7 (294 pixels: one whole staging chunk of 256 and 38 of the next) and one
probe of 128 (384 chunks), in batches of 1, 3 and 5 (one block per probe); colours log-uniform in 1e-3 .. 1e4. Mips, levels and RGBM at
S = 16 and 32 on two probes of different content: a smooth gradient (with a subnormal block and a negative channel) and the same with one
texel at 1e4.

Levels 1 .. 4: `e32` is the largest difference between the oracle run in float32 and in float64, divided by the level's largest value,
recorded per case, probe and level in the fixture; the device must lie within 4 x e32 of the float64 oracle. The factor covers a
different sum order and the device's log2, each rounding noise of that size; one wrong sample of 128 is orders larger
(tests/test_probes_cpu.py)."""
import os

import numpy as np
import pytest

from tests import probe_oracle as PO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probes_small.npz")
_expected = {}
INVALID, CAPACITY, NOT_BUILT = 1, 5, 6


def expected(name):
    """the oracle's outputs of a case, computed once and shared (read-only)"""
    if name not in _expected:
        r = PO.run_case(PO.cases()[name])
        for v in r.values():
            v.setflags(write=False)
        _expected[name] = r
    return _expected[name]


def bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    if a.tobytes() != b.tobytes():
        view = np.uint8 if a.itemsize == 1 else np.uint32
        bad = np.nonzero(np.ascontiguousarray(a).reshape(-1).view(view) != np.ascontiguousarray(b).reshape(-1).view(view))[0]
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at {bad[:5]}: {a.reshape(-1)[bad[:5]]} vs {b.reshape(-1)[bad[:5]]}")


def refused(api, code, fn, *args):
    with pytest.raises(api.LumixError) as e:
        fn(*args)
    assert e.value.code == code, e.value


@pytest.mark.parametrize("name", list(PO.cases()))
def test_sh_matches_oracle_and_reference(gpu_ctx, name):
    from lumixengine_amd import api

    c = PO.cases()[name]
    pb = api.ProbeBaker(gpu_ctx)
    pb.setCubemaps(c["cubemaps"])
    pb.shRun()
    got = pb.readSH()
    bits(got, expected(name)["sh"], f"{name}: sh against the oracle")
    bits(got, np.load(GOLDEN)[f"{name}|sh"], f"{name}: sh against the reference's record")
    assert np.isfinite(got).all() and (got[:, 0] > 0).all()
    pb.shRun()  # the table of this size is kept: the same again
    bits(pb.readSH(), got, f"{name}: a second run")
    d = pb.deviceOutputs()
    assert d.d_sh and d.d_cubemaps and not d.d_mips and d.n == len(got)
    pb.close()


def test_sh_batches_of_different_sizes_on_one_baker(gpu_ctx):
    """S = 5, then 16, then 5 again: the per-size table is rebuilt, and a smaller batch behind a larger one reads its own probes"""
    from lumixengine_amd import api

    pb = api.ProbeBaker(gpu_ctx)
    for name in ("sh S=5 n=5", "sh S=16 n=5", "sh S=2 n=3", "sh S=5 n=5"):
        pb.setCubemaps(PO.cases()[name]["cubemaps"])
        pb.shRun()
        bits(pb.readSH(), expected(name)["sh"], name)
    pb.close()


@pytest.mark.parametrize("name", [k for k, c in PO.cases().items() if c["mips"]])
def test_mips_bit_equal(gpu_ctx, name):
    from lumixengine_amd import api

    c, want = PO.cases()[name], expected(name)
    pb = api.ProbeBaker(gpu_ctx)
    pb.setCubemaps(c["cubemaps"])
    pb.mipsRun()
    got = pb.readMips()
    g = np.load(GOLDEN)
    n_mips = c["cubemaps"].shape[2].bit_length() - 1
    for p in range(len(got)):
        assert len(got[p]) == n_mips
        for m in range(n_mips):
            bits(got[p][m], want[f"mip{m + 1}"][p], f"{name}: probe {p} mip {m + 1} against the oracle")
            bits(got[p][m], g[f"{name}|mip{m + 1}"][p], f"{name}: probe {p} mip {m + 1} against the reference harness's record")
    if name.startswith("gradient"):
        sub = want["mip1"][0, 1, 1, 1, 3]
        assert 0 < sub < np.finfo(np.float32).tiny, "the subnormal block's average is kept"
    pb.close()


def sampler_queries(S):
    """directions on face centres, edges and corners, axis ties, half-texel offsets, random ones; lods 0, fractional, 4, past the chain"""
    rng = np.random.default_rng(11)
    d = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]  # face centres
    d += [(1, 1, 0), (1, -1, 0), (-1, 0, 1), (0, 1, 1), (0, -1, 1), (1, 0, -1), (0, 2, -2), (-3, 3, 0)]  # edges: two-axis ties
    d += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]  # corners: three-axis ties
    d += [(1, 0.999999, 0.5), (0.3, -1, 1.0000001), (1, 1 - 1 / S, 1 - 1 / S), (-1, 1 - 2 / S, -1 + 1 / S)]
    for f in range(6):  # texel centres, and points half a texel off in x, in y, in both: on the edges of the face too
        for x, y in ((0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1), (S // 2, S // 3)):
            for ox, oy in ((0.5, 0.5), (0, 0.5), (0.5, 0), (0, 0), (1, 1), (1, 0.5)):
                a, b = (x + ox) / S * 2 - 1, (y + oy) / S * 2 - 1
                v = PO.face_dir(np.array([f]), np.array([a], np.float32), np.array([b], np.float32))
                d.append(tuple(float(k[0]) * 3.5 for k in v))
    d = np.concatenate([np.array(d, np.float32), rng.normal(size=(200, 3)).astype(np.float32)])
    top = S.bit_length() - 1
    lods = np.array([0.0, 0.37, 1.0, 2.5, 3.999, 4.0, top - 0.25, top, top + 0.5, 100.0, -1.0], np.float32)
    dirs = np.repeat(d, len(lods), axis=0)
    return dirs, np.tile(lods, len(d))


@pytest.mark.parametrize("name", ["gradient S=16", "gradient S=32"])
def test_sampler_bit_equal(gpu_ctx, name):
    from lumixengine_amd import api

    cm = PO.cases()[name]["cubemaps"]
    S = cm.shape[2]
    pb = api.ProbeBaker(gpu_ctx)
    pb.setCubemaps(cm)
    pb.mipsRun()
    dirs, lods = sampler_queries(S)
    for p in range(2):
        chain = [cm[p]] + [expected(name)[f"mip{m}"][p] for m in range(1, S.bit_length())]
        want = PO.sample(chain, dirs, lods)
        bits(pb.sample(p, dirs, lods), want, f"{name}: probe {p}")
        assert np.isfinite(want).all()
    pb.close()


@pytest.mark.parametrize("name", [k for k, c in PO.cases().items() if c.get("filter")])
def test_levels_and_rgbm(gpu_ctx, name):
    from lumixengine_amd import api

    c, want = PO.cases()[name], expected(name)
    cm = c["cubemaps"]
    pb = api.ProbeBaker(gpu_ctx)
    pb.setCubemaps(cm)
    pb.filterRun()
    levels, rgbm, mips = pb.readFiltered(), pb.readRGBM(), pb.readMips()
    g = np.load(GOLDEN)
    for p in range(len(cm)):
        bits(mips[p][0], want["mip1"][p], f"{name}: probe {p} mip 1 behind filter_run")
        expect0 = cm[p].copy()
        expect0[..., 3] = 1.0
        bits(levels[p][0], expect0, f"{name}: probe {p} level 0 against mip 0")
        exact = PO.filter_levels(cm[p], T=np.float64)
        for k in range(1, 5):
            got = levels[p][k]
            assert got.shape == exact[k].shape and (got[..., 3] == 1.0).all()
            top = np.abs(exact[k][..., :3]).max()
            err = np.abs(got[..., :3].astype(np.float64) - exact[k][..., :3]).max() / top
            e32 = float(g[f"{name}|e32"][p, k - 1])
            live = np.abs(want[f"level{k}"][p][..., :3].astype(np.float64) - exact[k][..., :3]).max() / top
            print(f"{name} probe {p} level {k}: device error {err:.3e}, e32 recorded {e32:.3e}, e32 here {live:.3e}")
            assert err <= 4 * e32, f"{name} probe {p} level {k}: {err:.3e} against 4 x {e32:.3e}"
        want_rgbm = PO.oracle_rgbm(levels[p])
        for f in range(6):
            for k in range(5):
                bits(rgbm[p][f][k], want_rgbm[f][k], f"{name}: probe {p} face {f} level {k} RGBM of the device's floats")
    d = pb.deviceOutputs()
    assert d.d_filtered and d.d_rgbm and d.d_mips
    pb.close()


def test_rgbm_clamp_routes(gpu_ctx):
    """level 0 is mip 0, so its RGBM bytes are saveCubemap's of the input: negative channels, m below 1 / 64 and above 4, 0.5 ties"""
    from lumixengine_amd import api

    cm = PO.rgbm_routes()[None]
    pb = api.ProbeBaker(gpu_ctx)
    pb.setCubemaps(cm)
    pb.filterRun()
    got = pb.readRGBM()[0]
    for f in range(6):
        bits(got[f][0], PO.rgbm_texels(cm[0, f]), f"face {f}")
    g = np.load(GOLDEN)
    bits(np.stack([got[f][0] for f in range(6)]), g["rgbm routes|rgbm"], "against the reference's record")
    a = np.stack([got[f][0][..., 3] for f in range(6)])
    assert a.min() == 1 and a.max() == 255 and (np.stack([got[f][0][..., :3] for f in range(6)]) == 0).any()
    pb.close()


def test_refusals(gpu_ctx):
    from lumixengine_amd import api

    pb = api.ProbeBaker(gpu_ctx)
    for fn in (pb.shRun, pb.mipsRun, pb.filterRun, pb.readSH, pb.readMips, pb.readFiltered, pb.readRGBM, pb.deviceOutputs):
        refused(api, NOT_BUILT, fn)
    refused(api, NOT_BUILT, pb.sample, 0, np.ones((1, 3), np.float32), np.zeros(1, np.float32))
    refused(api, INVALID, pb.setCubemaps, np.zeros((0, 6, 4, 4, 4), np.float32))  # n == 0
    refused(api, INVALID, pb.setCubemaps, np.zeros((2, 6, 0, 0, 4), np.float32))  # S == 0
    for bad in (np.nan, np.inf, -np.inf):
        for ch in range(4):
            cm = np.ones((2, 6, 3, 3, 4), np.float32)
            cm[1, 5, 2, 2, ch] = bad
            refused(api, INVALID, pb.setCubemaps, cm)
    # above the byte cap: refused before the array is read (a small array stands for the batch)
    one = np.ones((1, 6, 1, 1, 4), np.float32)
    rc = pb.lib.lmx_probes_set_cubemaps(pb.h, 1 << 22, 128, one.ctypes.data)
    assert rc == CAPACITY
    assert pb.lib.lmx_probes_set_cubemaps(pb.h, 1, 1 << 20, one.ctypes.data) == CAPACITY
    assert pb.lib.lmx_probes_set_cubemaps(pb.h, 0xFFFFFFFF, 0xFFFFFFFF, one.ctypes.data) == CAPACITY
    assert api.probes_batch_bytes(682, 128) == 682 * 6 * 128 * 128 * 16 <= api.PROBES_MAX_BATCH_BYTES
    with pytest.raises(api.LumixError) as e:
        api.probes_batch_bytes(683, 128)
    assert e.value.code == CAPACITY
    refused(api, NOT_BUILT, pb.shRun)  # a refused batch left nothing behind
    # the filter's sizes: a power of two of 16 or more
    for S in (1, 5, 8, 24):
        pb.setCubemaps(np.ones((1, 6, S, S, 4), np.float32))
        pb.shRun()
        refused(api, INVALID, pb.mipsRun)
        refused(api, INVALID, pb.filterRun)
        refused(api, NOT_BUILT, pb.readMips)
        refused(api, NOT_BUILT, pb.readFiltered)
    pb.setCubemaps(np.ones((2, 6, 16, 16, 4), np.float32))
    refused(api, NOT_BUILT, pb.readSH)  # a new batch drops the outputs of the one before
    refused(api, NOT_BUILT, pb.sample, 0, np.ones((1, 3), np.float32), np.zeros(1, np.float32))
    pb.mipsRun()
    refused(api, NOT_BUILT, pb.readFiltered)
    refused(api, INVALID, pb.sample, 2, np.ones((1, 3), np.float32), np.zeros(1, np.float32))  # probe 2 of 2
    refused(api, INVALID, pb.sample, 0, np.zeros((1, 3), np.float32), np.zeros(1, np.float32))  # a zero direction
    refused(api, INVALID, pb.sample, 0, np.array([[1, np.nan, 0]], np.float32), np.zeros(1, np.float32))
    refused(api, INVALID, pb.sample, 0, np.ones((1, 3), np.float32), np.array([np.inf], np.float32))
    out = np.zeros(27, np.float32)
    pb.shRun()
    assert pb.lib.lmx_probes_read_sh(pb.h, out.ctypes.data, 1) == CAPACITY  # two probes
    assert pb.lib.lmx_probes_read_mips(pb.h, out.ctypes.data, 27) == CAPACITY
    with pytest.raises(api.LumixError):
        api.probes_ggx_samples(5)
    pb.close()
