"""Pins tests/texcomp_oracle.py to the reference's own encoder (CPU; skipped where the reference tree is absent).

A harness written here includes the reference's external/rgbcx/rgbcx.h in a temporary directory (nothing of it is committed) and is built
with g++ -O2 -msse2 -mfpmath=sse -ffp-contract=off. It encodes blocks at level 10 and in the exhaustive mode, with and without 3-colour
blocks, encodes BC4 / BC5, and dumps the two tables of likely total orderings with the order of the histograms they index.

  - The oracle given the reference's 20 (3 colours: 8) likely histograms of a block, in the reference's order, equals the level-10 bytes
    bit for bit; given all 969 (153) in the reference's order it equals the exhaustive bytes. That pins the whole flow; only the order in
    which the histograms are tried is this library's own.
  - In its own lexicographic order the oracle's per-block error equals the reference's exhaustive error exactly and is <= the level-10
    error, on every fixture block and every seeded one.
  - BC4 equals the reference's on every (min, max) pair with all values between.
  - The derived tables (midpoints, single-colour matches) equal the reference's; the committed fixture is what the reference gives.
"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests import texcomp_oracle as TO

REF = "/root/reference"
RGBCX = os.path.join(REF, "external", "rgbcx")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texcomp_small.npz")
FLAGS = ["-std=c++17", "-O2", "-msse2", "-mfpmath=sse", "-ffp-contract=off", "-w"]

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(RGBCX, "rgbcx.h")) or shutil.which("g++") is None, reason="needs the reference tree and g++")

HARNESS = r"""
#include <cstring>
#include <cmath>
#include <cassert>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>
#define RGBCX_IMPLEMENTATION
#include "rgbcx.h"

static void put(FILE* o, const void* p, size_t n) { if (fwrite(p, 1, n, o) != n) exit(3); }

int main(int argc, char** argv) {
	rgbcx::init();
	if (!strcmp(argv[1], "tables")) {
		FILE* o = fopen(argv[2], "wb");
		put(o, rgbcx::g_unique_total_orders4, sizeof(rgbcx::g_unique_total_orders4));
		put(o, rgbcx::g_unique_total_orders3, sizeof(rgbcx::g_unique_total_orders3));
		for (uint32_t i = 0; i < rgbcx::NUM_UNIQUE_TOTAL_ORDERINGS4; ++i)
			for (uint32_t q = 0; q < 32; ++q) { const uint16_t v = rgbcx::g_best_total_orderings4[i][q]; put(o, &v, 2); }
		put(o, rgbcx::g_best_total_orderings3, sizeof(rgbcx::g_best_total_orderings3));
		put(o, rgbcx::g_midpoint5, sizeof(rgbcx::g_midpoint5));
		put(o, rgbcx::g_midpoint6, sizeof(rgbcx::g_midpoint6));
		put(o, rgbcx::g_bc1_match5_equals_1, 768);
		put(o, rgbcx::g_bc1_match6_equals_1, 768);
		put(o, rgbcx::g_bc1_match5_half, 768);
		put(o, rgbcx::g_bc1_match6_half, 768);
		fclose(o);
		return 0;
	}
	FILE* f = fopen(argv[2], "rb");
	FILE* o = fopen(argv[3], "wb");
	uint32_t n = 0;
	if (fread(&n, 4, 1, f) != 1) return 2;
	std::vector<uint8_t> px((size_t)n * 64);
	if (n && fread(px.data(), 64, n, f) != n) return 2;
	std::vector<uint8_t> out((size_t)n * 16);
	const uint32_t ex = rgbcx::cEncodeBC1TwoLeastSquaresPasses | rgbcx::cEncodeBC1UseLikelyTotalOrderings | rgbcx::cEncodeBC1Exhaustive;
	auto now = [] { return std::chrono::steady_clock::now(); };
	auto ns = [](auto a, auto b) { return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count(); };
	if (!strcmp(argv[1], "bc4")) {
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc4(&out[i * 8], &px[(size_t)i * 64], 4);
		put(o, out.data(), (size_t)n * 8);
	} else {
		auto t0 = now();
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc1(10, &out[i * 8], &px[(size_t)i * 64], false, false);
		auto t1 = now();
		put(o, out.data(), (size_t)n * 8);
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc1(10, &out[i * 8], &px[(size_t)i * 64], true, false);
		put(o, out.data(), (size_t)n * 8);
		auto t2 = now();
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc1(&out[i * 8], &px[(size_t)i * 64], ex, 32, 32);
		auto t3 = now();
		put(o, out.data(), (size_t)n * 8);
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc1(&out[i * 8], &px[(size_t)i * 64], ex | rgbcx::cEncodeBC1Use3ColorBlocks, 32, 32);
		put(o, out.data(), (size_t)n * 8);
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc4(&out[i * 8], &px[(size_t)i * 64], 4);
		put(o, out.data(), (size_t)n * 8);
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc5(&out[i * 16], &px[(size_t)i * 64]);
		put(o, out.data(), (size_t)n * 16);
		for (uint32_t i = 0; i < n; ++i) rgbcx::encode_bc3(10, &out[i * 16], &px[(size_t)i * 64]);
		put(o, out.data(), (size_t)n * 16);
		if (n) fprintf(stderr, "level10 %lld exhaustive %lld\n", ns(t0, t1) / n, ns(t2, t3) / n);
	}
	fclose(o);
	return 0;
}
"""


def build_harness(work):
    src = os.path.join(work, "texcomp_harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(work, "texcomp_harness")
    subprocess.run(["g++"] + FLAGS + ["-I" + RGBCX, src, "-o", exe], check=True)
    return exe


def ref_tables(ref):
    exe, work = ref
    path = os.path.join(work, "tables.bin")
    subprocess.run([exe, "tables", path], check=True)
    raw = np.fromfile(path, np.uint8)
    at = 0

    def take(n, dtype, shape):
        nonlocal at
        a = raw[at: at + n].view(dtype).reshape(shape)
        at += n
        return a

    t = dict(unique4=take(969 * 4, np.uint8, (969, 4)).astype(np.int64), unique3=take(153 * 3, np.uint8, (153, 3)).astype(np.int64),
             best4=take(969 * 32 * 2, "<u2", (969, 32)).astype(np.int64), best3=take(153 * 32, np.uint8, (153, 32)).astype(np.int64),
             mid5=take(128, "<f4", (32,)), mid6=take(256, "<f4", (64,)))
    for k in ("m5", "m6", "m5h", "m6h"):
        t[k] = take(768, np.uint8, (256, 3)).astype(np.int64)
    assert at == len(raw)
    return t


def ref_encode(ref, blocks, mode="encode"):
    """-> dict of the reference's bytes for blocks uint8 (N, 16, 4), and its times per block in ns (level 10, exhaustive)"""
    exe, work = ref
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 64)
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32(len(blocks)).tobytes())
        f.write(blocks.tobytes())
    r = subprocess.run([exe, mode, src, dst], check=True, capture_output=True, text=True)
    raw = np.fromfile(dst, np.uint8)
    n = len(blocks)
    if mode == "bc4":
        return raw.reshape(n, 8)
    out, at = {}, 0
    for key, per in (("l10_4", 8), ("l10_3", 8), ("ex_4", 8), ("ex_3", 8), ("bc4", 8), ("bc5", 16), ("bc3_l10", 16)):
        out[key] = raw[at: at + n * per].reshape(n, per)
        at += n * per
    words = r.stderr.split()
    out["ns"] = (int(words[1]), int(words[3])) if len(words) >= 4 else (0, 0)
    return out


def recorded(ref, blocks):
    """what tests/golden/texcomp_small.npz holds"""
    r = ref_encode(ref, blocks)
    out = {"rgba": blocks}
    for k in ("l10_4", "l10_3", "ex_4", "ex_3"):
        out[k] = r[k]
        out[k + "_err"] = TO.block_error(blocks, r[k]).astype(np.uint32)
    out["bc4"], out["bc5"] = r["bc4"], r["bc5"]
    return out


def seeded_blocks(n=20000):
    rng = np.random.default_rng(7)
    k = n // 5
    a, b = rng.integers(0, 256, (k, 1, 4)), rng.integers(0, 256, (k, 1, 4))
    g0, g1 = rng.integers(0, 256, (k, 1, 1)), rng.integers(0, 256, (k, 1, 1))
    kinds = [rng.integers(0, 256, (k, 16, 4)), np.clip(a + (b - a) * rng.random((k, 16, 1)) + rng.normal(0, 6, (k, 16, 4)), 0, 255),
             np.clip(rng.integers(0, 256, (k, 1, 4)) + rng.integers(-2, 3, (k, 16, 4)), 0, 255), np.broadcast_to(np.where(np.arange(16)[None, :, None] < 8, g0, g1), (k, 16, 4)),
             np.where(rng.integers(0, 2, (k, 16, 1)) == 1, a, b)]
    return np.ascontiguousarray(np.concatenate([x.astype(np.uint8) for x in kinds]))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("texcomp_ref"))
    return build_harness(work), work


@pytest.fixture(scope="module")
def rtab(ref):
    return ref_tables(ref)


@pytest.fixture(scope="module")
def world(ref):
    """all blocks (the fixture's, then the seeded ones), what the reference gives for them, and the oracle in its own order"""
    blocks = np.concatenate([TO.fixture_blocks(), seeded_blocks()])
    r = ref_encode(ref, blocks)
    t0 = time.time()
    own4, own3 = TO.encode_bc1_pair(blocks)
    print(f"\noracle, own order: {time.time() - t0:.1f} s for {len(blocks)} blocks; the reference, one thread: level 10 {r['ns'][0] / 1000:.2f} us per block, exhaustive {r['ns'][1] / 1000:.1f} us per block")
    return blocks, r, own4, own3


def _orders(rtab, count4, count3):
    """the oracle's order arguments: the reference's likely histograms of a block's histogram before the search (count None: all, in its order).
    The row of a histogram is hist4 / hist3::lookup_total_ordering_index (:1601-1657): the hash of the table's own rows, and for a histogram
    with a 16 the constants TOTAL_ORDER_*_16 - of which TOTAL_ORDER_3_1_16 = 15 names the row of (0, 0, 16) and TOTAL_ORDER_3_2_16 = 89 that of
    (0, 16, 0): level 10 looks the likely list of the one up for the other. Only this lookup sees that; the exhaustive mode has no lookup."""
    row4 = {tuple(h): i for i, h in enumerate(rtab["unique4"].tolist())}
    row3 = {tuple(h): i for i, h in enumerate(rtab["unique3"].tolist())}
    for k, row in enumerate((15, 700, 753, 515)):
        assert row4[tuple(16 if j == k else 0 for j in range(4))] == row
    row3.update({(16, 0, 0): 12, (0, 16, 0): 15, (0, 0, 16): 89})

    def order4(hist):
        if count4 is None:
            return np.broadcast_to(rtab["unique4"], (len(hist), 969, 4))
        rows = np.array([row4[tuple(h)] for h in hist.tolist()])
        return rtab["unique4"][rtab["best4"][rows, :count4]]

    def order3(hist):
        if count3 is None:
            return np.broadcast_to(rtab["unique3"], (len(hist), 153, 3))
        rows = np.array([row3[tuple(h)] for h in hist.tolist()])
        return rtab["unique3"][rtab["best3"][rows, :count3]]

    return order4, order3


def test_derived_tables_equal_the_references(rtab):
    t = TO.tables()
    assert t["mid5"].tobytes() == rtab["mid5"].tobytes() and t["mid6"].tobytes() == rtab["mid6"].tobytes(), "a derived midpoint rounds unlike the reference's literal"
    for k in ("m5", "m6", "m5h", "m6h"):
        assert np.array_equal(t[k], rtab[k]), k
    assert sorted(map(tuple, rtab["unique4"].tolist())) == list(map(tuple, TO.hist4_list().tolist()))
    assert sorted(map(tuple, rtab["unique3"].tolist())) == list(map(tuple, TO.hist3_list().tolist()))


def test_level_10_bit_for_bit(world, rtab):
    blocks, r, _, _ = world
    order4, order3 = _orders(rtab, 20, 8)
    (got4, _), (got3, _) = TO.encode_bc1_pair(blocks, order4=order4, order3=order3)
    assert np.array_equal(got4, r["l10_4"]), f"{(got4 != r['l10_4']).any(1).sum()} blocks differ from level 10 (4 colours)"
    assert np.array_equal(got3, r["l10_3"]), f"{(got3 != r['l10_3']).any(1).sum()} blocks differ from level 10 (3 colours allowed)"
    bc3 = np.concatenate([TO.encode_bc4(blocks[:, :, 3]), got4], 1)
    assert np.array_equal(bc3, r["bc3_l10"])


def test_exhaustive_in_the_references_order_bit_for_bit(world, rtab):
    blocks, r, _, _ = world
    order4, order3 = _orders(rtab, None, None)
    (got4, _), (got3, _) = TO.encode_bc1_pair(blocks, order4=order4, order3=order3)
    assert np.array_equal(got4, r["ex_4"]), f"{(got4 != r['ex_4']).any(1).sum()} blocks differ from the exhaustive mode (4 colours)"
    assert np.array_equal(got3, r["ex_3"]), f"{(got3 != r['ex_3']).any(1).sum()} blocks differ from the exhaustive mode (3 colours allowed)"


def test_own_order_error_equals_exhaustive_and_is_within_level_10(world):
    blocks, r, own4, own3 = world
    for (got, err), ex, l10, name in ((own4, r["ex_4"], r["l10_4"], "4 colours"), (own3, r["ex_3"], r["l10_3"], "3 colours allowed")):
        mine = TO.block_error(blocks, got)
        assert np.array_equal(mine, TO.block_error(blocks, ex)), name
        assert (mine <= TO.block_error(blocks, l10)).all(), name
        solid = (blocks[:, :, :3] == blocks[:, :1, :3]).all((1, 2))
        assert np.array_equal(mine[~solid], err[~solid]), "the encoder's own count of the error is the decoder's"
    _, three = TO.decode_bc1(own4[0])
    assert not three.any(), "a 4-colour-only block has color0 > color1"


def test_bc4_on_every_min_max_pair(ref):
    vals = []
    for mn in range(256):
        for mx in range(mn, 256):
            between = np.arange(mn, mx + 1)
            for at in range(0, len(between), 14):
                chunk = between[at: at + 14]
                vals.append(np.concatenate([[mn, mx], chunk, np.full(14 - len(chunk), mn)]))
    vals = np.array(vals, np.uint8)
    blocks = np.zeros((len(vals), 16, 4), np.uint8)
    blocks[:, :, 0] = vals
    assert np.array_equal(TO.encode_bc4(vals), ref_encode(ref, blocks, "bc4"))


def test_bc5_equals_the_references(world):
    blocks, r, _, _ = world
    assert np.array_equal(TO.encode(blocks, TO.BC5)[0], r["bc5"]) and np.array_equal(TO.encode(blocks, TO.BC4)[0], r["bc4"])


def test_fixture_is_what_the_reference_gives(ref):
    g = np.load(GOLDEN)
    blocks = TO.fixture_blocks()
    assert np.array_equal(g["rgba"], blocks)
    now = recorded(ref, blocks)
    assert sorted(g.files) == sorted(now)
    for k in g.files:
        assert np.array_equal(g[k], now[k]), k
