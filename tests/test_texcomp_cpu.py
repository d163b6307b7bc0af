"""The texture compressor without a device: the host-only entry points and their refusals, the generated tables, the kernels' arithmetic
run on the host (lmx_texcomp_encode_host) against tests/texcomp_oracle.py and the reference's record, the oracle's one-rule mutants, and
csrc/lmx_texcomp.h's host side under sanitizers."""
import os

import numpy as np
import pytest

from tests import texcomp_oracle as TO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texcomp_small.npz")
INVALID, CAPACITY = 1, 5


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
    """the oracle on the fixture, in its own order: ((bytes, err) without 3-colour blocks, (bytes, err) with); computed once, read-only"""
    res = TO.encode_bc1_pair(golden["rgba"])
    for pair in res:
        for v in pair:
            v.setflags(write=False)
    return res


def test_output_bytes_and_refusals(api):
    assert api.texcomp_output_bytes([(4, 4)], api.TEX_BC1) == 8 and api.texcomp_output_bytes([(4, 4)], api.TEX_BC3) == 16
    assert api.texcomp_output_bytes([(1, 1), (5, 4), (4, 9)], api.TEX_BC4) == 8 * (1 + 2 + 3) and api.texcomp_output_bytes([(4096, 4096)], api.TEX_BC5) == 16 << 20
    # a probe's .lbc payload: six faces of levels 128 .. 8
    assert api.texcomp_output_bytes([(128 >> k, 128 >> k) for _ in range(6) for k in range(5)], api.TEX_BC3) == 16 * 6 * (1024 + 256 + 64 + 16 + 4)
    for sizes, fmt, code in (([], 0, INVALID), ([(0, 4)], 0, INVALID), ([(4, 4), (4, 0)], 0, INVALID), ([(4, 4)], 4, INVALID), ([(4, 4)], -1, INVALID),
                             ([(16384, 16385)], 0, CAPACITY), ([(16384, 16384)] + [(1, 1)], 0, CAPACITY), ([(0xffffffff, 0xffffffff)], 0, CAPACITY)):
        with pytest.raises(api.LumixError) as e:
            api.texcomp_output_bytes(sizes, fmt)
        assert e.value.code == code, (sizes, fmt)
    assert api.texcomp_output_bytes([(16384, 16384)], 0) == 8 << 24, "exactly LMX_TEXCOMP_MAX_BATCH_BYTES of pixels is let through"
    lib = api.load_library()
    d = np.array([[4, 4]], np.uint32)
    assert lib.lmx_texcomp_output_bytes(1, d.ctypes.data, 0, None) == INVALID and lib.lmx_texcomp_tables(None, 1 << 20) == INVALID
    assert lib.lmx_texcomp_tables(np.zeros(8, np.uint8).ctypes.data, 8) == INVALID
    for h in ([16, 1, 0, 0], [0, 0, 0], [5, 5, 5, 2]):
        with pytest.raises(api.LumixError):
            api.texcomp_hist_index(h)
    assert lib.lmx_texcomp_encode_host(7, 0, d.ctypes.data, d.ctypes.data, None) == INVALID and lib.lmx_texcomp_encode_host(0, 1, None, d.ctypes.data, None) == INVALID


def test_blocks_per_round_is_the_documented_grid(api):
    """at most 1024 workgroups of four waves, one block per wave; tests/test_gpu_texcomp.py sizes its grid-stride case from
    this value, and the kernel's source holds the same constants"""
    assert api.texcomp_blocks_per_round() == 1024 * 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "lumixengine_amd", "csrc", "lmx_texcomp.h")).read()
    assert "TC_MAX_GRID = 1024;" in header and "TC_BLOCK = 256;" in header and "TC_BLOCKS_PER_ROUND = TC_MAX_GRID * TC_WAVES;" in header
    kernels = open(os.path.join(root, "lumixengine_amd", "csrc", "texcomp_kernels.hip")).read()
    assert "want < TC_MAX_GRID ? want : TC_MAX_GRID" in kernels and "b += gridDim.x * TC_WAVES" in kernels


def test_generated_tables(api):
    t = api.texcomp_tables()
    assert api.TEX_TABLES.itemsize == 22432
    h4, h3 = TO.hist4_list(), TO.hist3_list()
    assert len(h4) == 969 and len(h3) == 153 and (h4.sum(1) == 16).all() and (h3.sum(1) == 16).all()
    for hists, table in ((h4, t["hist4"]), (h3, t["hist3"])):
        for i, h in enumerate(hists.tolist()):  # histogram <-> index, both ways
            assert api.texcomp_hist_index(h) == i == TO.hist_index(h)
        f = table["f"]
        if hists.shape[1] == 4:
            assert np.array_equal(f & 255, hists[:, 0]) and np.array_equal((f >> 8) & 255, hists[:, :2].sum(1)) and np.array_equal((f >> 16) & 255, hists[:, :3].sum(1))
        else:  # BC1's 3-colour order along the axis is selector 0, 2, 1
            assert np.array_equal(f & 255, hists[:, 0]) and np.array_equal((f >> 8) & 255, hists[:, 0] + hists[:, 2])
        all16 = np.flatnonzero(f >> 24)
        assert np.array_equal(all16, np.flatnonzero((hists == 16).any(1))) and len(all16) == hists.shape[1]
        iz00, iz10, iz11 = TO.selector_factors(hists)
        assert table["iz00"].tobytes() == iz00.tobytes() and table["iz10"].tobytes() == iz10.tobytes() and table["iz11"].tobytes() == iz11.tobytes()
        assert (table["iz00"][all16] == 0).all() and (table["iz11"][all16] == 0).all()
    o = TO.tables()
    assert t["mid5"].tobytes() == o["mid5"].tobytes() and t["mid6"].tobytes() == o["mid6"].tobytes()
    for k, name in enumerate(("m5", "m6", "m5h", "m6h")):
        m = t["match"][k].astype(np.int64)
        assert np.array_equal(np.stack([m & 255, (m >> 8) & 255, m >> 16], 1), o[name]), name
    assert o["m5"][0].tolist() == [0, 0, 0] and o["m5"][255].tolist() == [31, 31, 0], "black and white are matched exactly by coinciding endpoints"


def test_oracle_matches_the_reference_record(golden, own):
    blocks = golden["rgba"]
    assert np.array_equal(blocks, TO.fixture_blocks()) and len(blocks) <= 2048
    for (got, err), key in zip(own, ("4", "3")):
        mine = TO.block_error(blocks, got)
        assert np.array_equal(mine, golden[f"ex_{key}_err"]), "the per-block error is the exhaustive mode's, no block left out"
        assert (mine <= golden[f"l10_{key}_err"]).all() and (mine < golden[f"l10_{key}_err"]).mean() > 0.2
        assert np.array_equal(golden[f"ex_{key}_err"], TO.block_error(blocks, golden[f"ex_{key}"]))
        solid = (blocks[:, :, :3] == blocks[:, :1, :3]).all((1, 2))
        assert np.array_equal(mine[~solid], err[~solid]) and solid.sum() > 50
        assert np.array_equal(got[solid], golden[f"ex_{key}"][solid]), "solid blocks have no search: byte for byte the reference's"
    assert not TO.decode_bc1(own[0][0])[1].any() and TO.decode_bc1(own[1][0])[1].any()
    assert np.array_equal(TO.encode_bc4(blocks[:, :, 0]), golden["bc4"]) and np.array_equal(TO.encode(blocks, TO.BC5)[0], golden["bc5"])


def test_host_arithmetic_is_the_oracles(api, golden, own):
    """csrc/lmx_texcomp.h run on the host, block after block, bit for bit the oracle: what the kernels compute, before any device"""
    blocks = golden["rgba"]
    (o4, e4), (o3, e3) = own
    got, err = api.texcomp_encode_host(api.TEX_BC1, blocks)
    assert np.array_equal(got, o3) and np.array_equal(err, e3)
    got, err = api.texcomp_encode_host(api.TEX_BC3, blocks)
    assert np.array_equal(got[:, 8:], o4) and np.array_equal(err, e4) and np.array_equal(got[:, :8], TO.encode_bc4(blocks[:, :, 3]))
    assert np.array_equal(api.texcomp_encode_host(api.TEX_BC4, blocks)[0], golden["bc4"]) and np.array_equal(api.texcomp_encode_host(api.TEX_BC5, blocks)[0], golden["bc5"])
    assert api.texcomp_encode_host(api.TEX_BC1, np.zeros((0, 16, 4), np.uint8))[0].shape == (0, 8)


def test_the_fixture_takes_its_routes(golden):
    blocks = golden["rgba"]
    before = dict(TO.STATS)
    sub = blocks[1500:]  # the edge-case kinds
    TO.encode_bc1(sub, True)
    assert TO.STATS["clamped"] > before["clamped"] and TO.STATS["det0"] > before["det0"], "no rounding left [0, 31] / [0, 63], or no determinant was 0"
    solid = golden["ex_4"][(blocks[:, :, :3] == blocks[:, :1, :3]).all((1, 2))]
    sels = solid[:, 4:].view("<u4")[:, 0]
    assert {0, 0x55555555, 0xAAAAAAAA} <= set(sels.tolist()), "solid blocks through mask 0, the 0x55 route and the plain 0xAA"
    px = blocks[:, :, :3].astype(int)
    grey = ((px[:, :, 0] == px[:, :, 1]) & (px[:, :, 0] == px[:, :, 2])).all(1) & ~(px == px[:, :1]).all((1, 2))
    rng = px[:, :, 0].max(1) - px[:, :, 0].min(1)
    assert (grey & (rng < 2)).any() and (grey & (rng >= 2)).any()
    assert ((px.max(2) < 4).any(1) & (px.max((1, 2)) > 100)).any(), "dark pixels among bright ones"


# a subset that holds every kind and keeps a mutant's run short
def _subset(n):
    return np.unique(np.concatenate([np.arange(0, n, 8), np.arange(1500, n)]))


@pytest.mark.parametrize("rule", TO.MUTANTS)
def test_mutant_changes_a_block(golden, own, rule):
    blocks = golden["rgba"]
    idx = _subset(len(blocks))
    (m4, me4), (m3, me3) = TO.encode_bc1_pair(blocks[idx], mutant=rule)
    (o4, e4), (o3, e3) = own
    changed = (m4 != o4[idx]).any() or (m3 != o3[idx]).any() or (me4 != e4[idx]).any() or (me3 != e3[idx]).any()
    assert changed, f"no fixture block tells the rule '{rule}'"


def test_host_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """csrc/lmx_texcomp.h as host code - the tables, the whole block encoder at its edge routes, BC4, the batch's layout - in a stand-alone
    program (tests/cpp/texcomp_host_sanitize.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "texcomp_host_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "lumixengine_amd", "csrc"), os.path.join(root, "tests", "cpp", "texcomp_host_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
