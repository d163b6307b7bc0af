"""Mip chains without a device: the host utilities and their refusals, csrc/lmx_texmips.h's arithmetic run on the host (lmx_texmips_coeffs,
lmx_texmips_host) against tests/texmips_oracle.py and the reference's record (tests/golden/texmips_small.npz), the enumeration that keeps
downsampleNormal's index inside its row for sides up to 4096, the oracle's one-rule mutants, and the header's host side under sanitizers."""
import os

import numpy as np
import pytest

from tests import texmips_oracle as MO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texmips_small.npz")
INVALID, CAPACITY = 1, 5
SIZES = (("37x21", 37, 21), ("64x48", 64, 48), ("40x24", 40, 24))
MODE_NAMES = ((MO.LINEAR, "linear"), (MO.SRGB, "srgb"), (MO.STOCHASTIC, "stochastic"))
F = np.float32


@pytest.fixture(scope="module")
def api():
    from lumixengine_amd import api as a

    a.load_library()
    return a


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def own(golden):
    """the oracle's chains of the fixture images per (size, mode, coverage on); computed once, read-only"""
    out = {}
    for key, w, h in SIZES:
        for mode, _ in MODE_NAMES:
            for ref_norm in (-1.0, 0.5):
                v = MO.flatten(MO.chains(golden[f"{key}_images"], mode, ref_norm))
                v.setflags(write=False)
                out[key, mode, ref_norm] = v
    return out


def test_chain_levels_and_bytes(api):
    assert [api.texcomp_chain_levels(w, h) for w, h in ((1, 1), (2, 1), (3, 3), (4, 4), (37, 21), (4096, 4096), (4097, 1), (0, 4), (4, 0))] == [1, 2, 2, 3, 6, 13, 13, 0, 0]
    assert api.texcomp_chain_sizes(37, 21) == [(37, 21), (18, 10), (9, 5), (4, 2), (2, 1), (1, 1)] == MO.sizes(37, 21)
    assert api.texcomp_chain_bytes(1, 1, 1) == 4 and api.texcomp_chain_bytes(3, 4, 4) == 3 * 4 * 21 and api.texcomp_chain_bytes(2, 8, 1) == 2 * 4 * 15
    assert api.texcomp_chain_bytes(1, 4096, 4096) == 4 * sum(4 ** k for k in range(13))
    for n, w, h, code in ((0, 4, 4, INVALID), (1, 0, 4, INVALID), (1, 4, 0, INVALID), (1, 16384, 16384, CAPACITY), (7, 8192, 8192, CAPACITY), (65536, 2, 1, CAPACITY),
                          (1, 0xffffffff, 0xffffffff, CAPACITY), (1, (1 << 24) + 1, 1, CAPACITY), (1, 1, (1 << 24) + 1, CAPACITY)):
        with pytest.raises(api.LumixError) as e:
            api.texcomp_chain_bytes(n, w, h)
        assert e.value.code == code, (n, w, h)
    lib = api.load_library()
    assert lib.lmx_texcomp_chain_bytes(1, 4, 4, None) == INVALID
    rows = np.zeros(4, api.TEXMIP_ROW)
    assert api.TEXMIP_ROW.itemsize == 64
    assert lib.lmx_texmips_coeffs(4, 2, None, 4) == INVALID and lib.lmx_texmips_coeffs(0, 0, rows.ctypes.data, 4) == INVALID
    assert lib.lmx_texmips_coeffs(2, 4, rows.ctypes.data, 4) == INVALID, "no upsampling"
    assert lib.lmx_texmips_coeffs(16, 8, rows.ctypes.data, 4) == CAPACITY
    opt = api.LmxTexMipOptions(3, -1.0)
    px = np.zeros(64, np.uint8)
    assert lib.lmx_texmips_host(api.C.byref(opt), 1, 2, 2, px.ctypes.data, px.ctypes.data) == INVALID and lib.lmx_texmips_host(None, 1, 2, 2, px.ctypes.data, px.ctypes.data) == INVALID
    with pytest.raises(api.LumixError) as e:
        api.texmips_host(np.zeros((1, 1, 4097, 4), np.uint8), MO.STOCHASTIC)
    assert e.value.code == CAPACITY


def test_coefficients_are_the_oracles(api):
    pairs = [(1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (9, 4), (21, 10), (37, 18), (64, 32), (7, 7), (129, 64), (4096, 2048), (4097, 2048), (8191, 4095)]
    most = 0
    for n_in, n_out in pairs:
        rows = api.texmips_coeffs(n_in, n_out)
        n0, n, c = MO.coeffs(n_in, n_out)
        assert np.array_equal(rows["n0"], n0) and np.array_equal(rows["n"], n) and rows["c"].tobytes() == c.tobytes(), (n_in, n_out)
        assert (n0 + n <= n_in).all() and (np.diff(n0) >= 0).all()
        if n_in != n_out:
            sums = np.zeros(n_out, F)
            for k in range(MO.MAX_TAPS):
                sums = sums + c[:, k]
            assert np.abs(sums - 1).max() < 4e-7, "normalised"
        most = max(most, int(n.max()))
    assert most <= 10 < MO.MAX_TAPS, "after the edge fold no output of a halving keeps more than ten texels"
    n0, n, c = MO.coeffs(64, 32)
    assert n[16] == 8 and n0[16] == 2 * 16 - 3, "an exact 2 : 1 has 8 taps: texels 2 o - 3 .. 2 o + 4"
    assert n[0] == 5 and n0[0] == 0 and n[31] == 5 and n0[31] == 59, "the edges fold theirs onto the first and last texel"


def test_every_halving_fits_the_kernels_taps_and_window(api):
    """The level kernel holds 14 taps per output and a 48-texel source window per 16-output tile; the library refuses a level that needs
    more before any launch. Enumerated here: every side 2 .. 4200 halved, and sampled sides up to the largest admitted, 2^24 (above it a
    texel centre p + 0.5f is no longer exact in fp32 and the side is refused)."""
    assert api.texcomp_chain_bytes(1, 1 << 24, 1) == 4 * (2 ** 25 - 1)
    lib = api.load_library()
    rows = np.zeros(1, api.TEXMIP_ROW)
    assert lib.lmx_texmips_coeffs((1 << 24) + 1, 1 << 23, rows.ctypes.data, 1) != 0
    rng = np.random.default_rng(5)
    sides = list(range(2, 4201)) + [int(s) for s in rng.integers(4201, 1 << 20, 40)] + [(1 << 20) + 1, (1 << 22) - 1]
    taps = window = 0
    for side in sides:
        rows = api.texmips_coeffs(side, side >> 1)
        n0, end = rows["n0"].astype(np.int64), rows["n0"].astype(np.int64) + rows["n"]
        assert (np.diff(n0) >= 0).all() and end.max() <= side and rows["n"].min() >= 1, side
        first = n0[::16]
        last = np.maximum.reduceat(end, np.arange(0, len(end), 16))
        taps, window = max(taps, int(rows["n"].max())), max(window, int((last - first).max()))
    print(f"\nat most {taps} taps and a window of {window} texels over {len(sides)} sides")
    assert taps <= MO.MAX_TAPS and window <= 48, (taps, window)  # TM_MAX_TAPS and TM_WINDOW of csrc/lmx_texmips.h


def test_host_arithmetic_is_the_oracles(api, golden, own):
    """csrc/lmx_texmips.h run on the host, chain after chain, bit for bit the oracle: what the kernels compute, before any device"""
    for key, w, h in SIZES:
        for mode, _ in MODE_NAMES:
            for ref_norm in (-1.0, 0.5):
                got = api.texmips_host(golden[f"{key}_images"], mode, ref_norm)
                assert np.array_equal(got, own[key, mode, ref_norm]), (key, mode, ref_norm)
    one = np.full((2, 1, 1, 4), 9, np.uint8)
    assert np.array_equal(api.texmips_host(one, MO.SRGB, 0.5), one.reshape(2, 4)), "1 x 1: no level to make, level 0 is never scaled"


def test_oracle_against_the_reference_record(golden, own):
    """stochastic and coverage bit for bit (whole chains); filtered levels from the recorded previous level within 1, under the caps"""
    for key, w, h in SIZES:
        assert MO.compute_coverage(golden[f"{key}_images"][0], 0.5).tobytes() == golden[f"{key}_coverage"].tobytes()
        assert np.array_equal(own[key, MO.STOCHASTIC, -1.0], golden[f"{key}_stochastic"]) and np.array_equal(own[key, MO.STOCHASTIC, 0.5], golden[f"{key}_stochastic_cov"])
        assert not np.array_equal(golden[f"{key}_stochastic"], golden[f"{key}_stochastic_cov"])
    from lumixengine_amd import api as A

    for mode, name, cap in ((MO.LINEAR, "linear", 0.001), (MO.SRGB, "srgb", 0.02)):
        compared = differ = 0
        for key, w, h in SIZES:
            for tag, ref_norm in (("", -1.0), ("_cov", 0.5)):
                for chain in golden[f"{key}_{name}{tag}"]:
                    lv = A.texcomp_split_chain(chain, w, h)
                    for m in range(1, len(lv)):
                        mine = MO.compute_mip(lv[m - 1], lv[m].shape[1], lv[m].shape[0], mode)
                        if tag:
                            with np.errstate(all="ignore"):
                                scale = float(MO.coverage_scale(mine, ref_norm, golden[f"{key}_coverage"]))
                            mine = MO.scale_coverage(mine, ref_norm, golden[f"{key}_coverage"])
                        d = np.abs(mine.astype(int) - lv[m].astype(int))
                        if tag:  # scaleCoverage multiplies an alpha that may differ by 1: colour is held to 1, alpha to the factor's reach
                            assert d[:, :, :3].max() <= 1
                            if np.isfinite(scale):
                                assert d[:, :, 3].max() <= np.ceil(scale) + 1, (key, name, m, scale, int(d[:, :, 3].max()))
                            continue
                        assert d.max() <= 1, (key, name, m)
                        compared, differ = compared + d.size, differ + int((d != 0).sum())
        assert [compared, differ] == golden[f"share_{name}"].tolist()
        assert differ <= cap * compared, f"{name}: {differ} of {compared} bytes differ from stb's"


def test_stochastic_index_stays_inside_for_sides_up_to_4096():
    """downsampleNormal only ASSERTs isrc < w. With the draw at its largest possible value (r = rw: rand() * 2.328306435996595e-10 < 1) the
    index u32(i * rw) + (r > r0) + (r > r0 + 1) stays inside the row for every destination texel of every side 1 .. 4096 halved."""
    for w in range(1, 4097):
        dst = max(w >> 1, 1)
        rw = F(w) / F(dst)
        s = np.arange(dst, dtype=F) * rw
        whole = np.floor(s)
        r0 = F(1) - (s - whole)
        worst = whole.astype(np.int64) + (rw > r0) + (rw > (r0 + F(1)))
        assert worst.max() < w, w
    # ... and 4163 is the first odd side whose largest draw reads one texel past the row
    def past(w):
        dst = w >> 1
        rw = F(w) / F(dst)
        s = np.arange(dst, dtype=F) * rw
        r0 = F(1) - (s - np.floor(s))
        return int((np.floor(s).astype(np.int64) + (rw > r0) + (rw > (r0 + F(1)))).max()) >= w
    assert past(4163) and not any(past(w) for w in range(4097, 4163))


def _fixture_chains(golden, mode, ref_norm, mutant):
    return np.concatenate([MO.flatten(MO.chains(golden[f"{key}_images"], mode, ref_norm, mutant)).reshape(-1) for key, _, _ in SIZES])


MUTANT_CASES = {"vertical_first": (MO.LINEAR, -1.0), "no_edge_fold": (MO.LINEAR, -1.0), "no_normalisation": (MO.LINEAR, -1.0), "no_premultiplied": (MO.SRGB, -1.0),
                "draws_swapped": (MO.STOCHASTIC, -1.0), "coverage_per_image": (MO.STOCHASTIC, 0.5), "next_from_unscaled": (MO.LINEAR, 0.5)}


@pytest.mark.parametrize("rule", MO.MUTANTS)
def test_mutant_changes_a_fixture_byte(golden, own, rule):
    mode, ref_norm = MUTANT_CASES[rule]
    mutated = _fixture_chains(golden, mode, ref_norm, rule)
    plain = np.concatenate([own[key, mode, ref_norm].reshape(-1) for key, _, _ in SIZES])
    assert (mutated != plain).any(), f"no fixture byte tells the rule '{rule}'"


def test_host_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """csrc/lmx_texmips.h as host code - the tables, the coefficient builder at its edge sizes, whole levels in the three modes, the coverage
    walk at its edges - in a stand-alone program (tests/cpp/texmips_host_sanitize.cpp) built with AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "texmips_host_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "lumixengine_amd", "csrc"), os.path.join(root, "tests", "cpp", "texmips_host_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
