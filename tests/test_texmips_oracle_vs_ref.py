"""Pins tests/texmips_oracle.py to the reference's own mip code (CPU; skipped where the reference tree is absent).

A harness written here is built at test time in a temporary directory around the reference's external/stb/stb_image_resize2.h, around
downsampleNormal / computeCoverage / scaleCoverage cut out of renderer/editor/render_plugins.cpp, and around the generator cut out of
core/math.cpp (nothing of them is committed), with g++ -O2 -msse2 -mfpmath=sse -ffp-contract=off.

  - stochastic levels and coverage (the count, the factor, the rescaled alpha): bit for bit, and the reference's ASSERTs on its source
    index never fire on the shapes tried;
  - filtered levels, each computed from the reference's own previous level: every byte within 1 of stbir_resize_uint8_linear / _srgb, and at
    most 0.1 % (linear) / 2 % (sRGB) of the bytes differ at all - the caps keep a wrong coefficient from hiding behind "within 1"
    (DESIGN.md §4.24 states the shares measured);
  - the generated sRGB decode table equals stb's 256 literals;
  - the committed fixture is what the reference gives.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import texmips_oracle as MO

REF = "/root/reference"
STB = os.path.join(REF, "external", "stb")
PLUGINS = os.path.join(REF, "src", "renderer", "editor", "render_plugins.cpp")
MATH = os.path.join(REF, "src", "core", "math.cpp")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texmips_small.npz")
FLAGS = ["-std=c++17", "-O2", "-msse2", "-mfpmath=sse", "-ffp-contract=off", "-w"]
LINEAR_CAP, SRGB_CAP = 0.001, 0.02  # the share of bytes that may differ from stb's at all

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(STB, "stb_image_resize2.h")) or not os.path.exists(PLUGINS) or shutil.which("g++") is None,
                                reason="needs the reference tree and g++")

# what the cut-out functions lean on, restated just far enough for them to compile
PRELUDE = r"""
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define STB_IMAGE_RESIZE_IMPLEMENTATION
#include "stb_image_resize2.h"
typedef uint8_t u8; typedef uint32_t u32; typedef int32_t i32;
static int g_assert_failed = 0;
#define ASSERT(x) do { if (!(x)) g_assert_failed = 1; } while (0)
#define PROFILE_FUNCTION()
template <typename T> struct Span { T* b; T* e; T* begin() const { return b; } };
struct Color { u8 r, g, b, a; };
template <typename T> T minimum(T a, T b) { return a < b ? a : b; }
template <typename T> T maximum(T a, T b) { return a > b ? a : b; }
template <typename T1, typename T2, typename T3> T1 clamp(T1 value, T2 min_value, T3 max_value) { return minimum(maximum(value, min_value), max_value); }
namespace jobs { template <typename F> void forEach(i32 count, i32, const F& f) { for (i32 i = 0; i < count; ++i) f(i, i + 1); } }
struct RandomGenerator { RandomGenerator(u32 u, u32 v); u32 rand(); float randFloat(float from, float to); u32 u, v; };
"""

MAIN = r"""
static void put(FILE* o, const void* p, size_t n) { if (fwrite(p, 1, n, o) != n) exit(3); }
int main(int argc, char** argv) {
	FILE* o = fopen(argv[2], "wb");
	if (!strcmp(argv[1], "table")) { put(o, stbir__srgb_uchar_to_linear_float, 1024); fclose(o); return 0; }
	FILE* f = fopen(argv[1], "rb");
	long long ns[3] = {0, 0, 0}, px[3] = {0, 0, 0};
	for (;;) {
		u32 hd[5]; float fl[2];
		if (fread(hd, 4, 5, f) != 5) break;
		if (fread(fl, 4, 2, f) != 2) return 2;
		const u32 op = hd[0], w = hd[1], h = hd[2], dw = hd[3], dh = hd[4];
		std::vector<u8> src((size_t)w * h * 4), dst((size_t)dw * dh * 4 + 4);
		if (fread(src.data(), 1, src.size(), f) != src.size()) return 2;
		auto t0 = std::chrono::steady_clock::now();
		if (op == 0) stbir_resize_uint8_linear(src.data(), w, h, 0, dst.data(), dw, dh, 0, STBIR_RGBA);
		else if (op == 1) stbir_resize_uint8_srgb(src.data(), w, h, 0, dst.data(), dw, dh, 0, STBIR_RGBA);
		else if (op == 2) downsampleNormal(Span<const u8>{src.data(), src.data() + src.size()}, Span<u8>{dst.data(), dst.data() + dst.size()}, w, h, dw, dh);
		auto t1 = std::chrono::steady_clock::now();
		if (op <= 2) { ns[op] += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count(); px[op] += (long long)dw * dh; put(o, dst.data(), (size_t)dw * dh * 4); }
		else if (op == 3) { const float c = computeCoverage(Span<const u8>{src.data(), src.data() + src.size()}, w, h, fl[0]); put(o, &c, 4); }
		else { scaleCoverage(Span<u8>{src.data(), src.data() + src.size()}, w, h, fl[0], fl[1]); put(o, src.data(), src.size()); }
	}
	fclose(o);
	fprintf(stderr, "%d %lld %lld %lld %lld %lld %lld\n", g_assert_failed, ns[0], px[0], ns[1], px[1], ns[2], px[2]);
	return 0;
}
"""


def _cut(text, start):
    """the function that begins with `start`, up to its closing brace in column 0"""
    at = text.index(start)
    return text[at: text.index("\n}", at) + 3]


def build_harness(work):
    plugins, math_cpp = open(PLUGINS).read(), open(MATH).read()
    parts = [PRELUDE, _cut(math_cpp, "RandomGenerator::RandomGenerator(u32 u, u32 v)"), _cut(math_cpp, "u32 RandomGenerator::rand()"),
             _cut(math_cpp, "float RandomGenerator::randFloat(float from, float to)"), _cut(plugins, "static void downsampleNormal("),
             _cut(plugins, "static float computeCoverage("), _cut(plugins, "static void scaleCoverage("), MAIN]
    src = os.path.join(work, "texmips_harness.cpp")
    with open(src, "w") as f:
        f.write("\n".join(parts))
    exe = os.path.join(work, "texmips_harness")
    subprocess.run(["g++"] + FLAGS + ["-I" + STB, src, "-o", exe], check=True)
    return exe


OPS = {"linear": 0, "srgb": 1, "stochastic": 2, "coverage": 3, "scale": 4}


def ref_run(ref, jobs):
    """jobs: (op name, uint8 (h, w, 4), ref_norm, wanted) -> the reference's result per job (an image, or the coverage), and its stderr line"""
    exe, work = ref
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        for op, img, a, b in jobs:
            h, w = img.shape[:2]
            f.write(np.array([OPS[op], w, h, max(w >> 1, 1), max(h >> 1, 1)], np.uint32).tobytes())
            f.write(np.array([a, b], np.float32).tobytes())
            f.write(np.ascontiguousarray(img, np.uint8).tobytes())
    r = subprocess.run([exe, src, dst], check=True, capture_output=True, text=True)
    raw, at, out = np.fromfile(dst, np.uint8), 0, []
    for op, img, _, _ in jobs:
        h, w = img.shape[:2]
        if op == "coverage":
            out.append(raw[at: at + 4].view("<f4")[0])
            at += 4
            continue
        oh, ow = (h, w) if op == "scale" else (max(h >> 1, 1), max(w >> 1, 1))
        out.append(raw[at: at + oh * ow * 4].reshape(oh, ow, 4))
        at += oh * ow * 4
    assert at == len(raw)
    return out, [int(x) for x in r.stderr.split()]


def ref_chain(ref, img, mode, scale_coverage_ref=-1.0, wanted=None):
    """the reference's loop for one image (:374-393): computeMip of the previous level, scaleCoverage behind it; -> the levels, 0 included"""
    chain = [img]
    while chain[-1].shape[0] > 1 or chain[-1].shape[1] > 1:
        (mip,), _ = ref_run(ref, [(mode, chain[-1], 0, 0)])
        if scale_coverage_ref >= 0:
            (mip,), _ = ref_run(ref, [("scale", mip, scale_coverage_ref, wanted)])
        chain.append(mip)
    return chain


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
FIXTURE_SIZES = ((37, 21), (64, 48), (40, 24))  # (w, h): odd ratios on both axes; exact 2 : 1 over several tiles; a ramp whose 2 : 1 averages are half-integers, where the order of the sums shows
FIXTURE_REF = 0.5


def fixture_images(w, h):
    """noise, a smooth ramp, and an image with a block of zero alpha"""
    rng = np.random.default_rng(w * 1000 + h)
    noise = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    ramp = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1), 255 - x * 200 // max(w - 1, 1)], 2).astype(np.uint8)
    hole = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    hole[h // 4: h // 4 + h // 2, w // 3: w // 3 + w // 2, 3] = 0
    return np.stack([noise, ramp, hole])


def shares(own, theirs):
    """(bytes compared, bytes that differ, the largest difference)"""
    d = np.abs(own.astype(int) - theirs.astype(int))
    return d.size, int((d != 0).sum()), int(d.max()) if d.size else 0


def recorded(ref):
    """what tests/golden/texmips_small.npz holds: per size the three images, the reference's chains in each mode without and with coverage
    scaling (the wanted coverage from image 0), its coverage, and the shares of bytes at which the oracle's filtered levels differ"""
    out = {}
    total = {"linear": [0, 0], "srgb": [0, 0]}
    for w, h in FIXTURE_SIZES:
        images = fixture_images(w, h)
        key = f"{w}x{h}"
        out[f"{key}_images"] = images
        (wanted,), _ = ref_run(ref, [("coverage", images[0], FIXTURE_REF, 0)])
        out[f"{key}_coverage"] = np.float32(wanted)
        for mode in ("linear", "srgb", "stochastic"):
            for tag, ref_norm in (("", -1.0), ("_cov", FIXTURE_REF)):
                chains = [ref_chain(ref, img, mode, ref_norm, wanted) for img in images]
                out[f"{key}_{mode}{tag}"] = MO.flatten(chains)
                if mode != "stochastic" and not tag:
                    for chain in chains:
                        for prev, lv in zip(chain, chain[1:]):
                            n, differ, worst = shares(MO.compute_mip(prev, lv.shape[1], lv.shape[0], OPS[mode]), lv)
                            assert worst <= 1
                            total[mode][0] += n
                            total[mode][1] += differ
    out["share_linear"] = np.array(total["linear"], np.int64)  # (bytes compared, bytes that differ)
    out["share_srgb"] = np.array(total["srgb"], np.int64)
    return out


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("texmips_ref"))
    return build_harness(work), work


def test_decode_table_is_stbs_256_of_256(ref):
    exe, work = ref
    path = os.path.join(work, "table.bin")
    subprocess.run([exe, "table", path], check=True)
    theirs = np.fromfile(path, "<f4")
    assert len(theirs) == 256 and int((MO.tables()[0] == theirs).sum()) == 256
    assert re.search(r"stbir__srgb_uchar_to_linear_float\[256\]", open(os.path.join(STB, "stb_image_resize2.h")).read())


STOCHASTIC_SHAPES = ((2, 1), (1, 2), (3, 3), (5, 5), (7, 3), (8, 8), (37, 21), (33, 17), (128, 64), (255, 3), (4096, 2), (3, 4095), (1023, 1025))


def test_stochastic_levels_bit_for_bit(ref):
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for w, h in STOCHASTIC_SHAPES]
    got, err = ref_run(ref, [("stochastic", im, 0, 0) for im in images])
    assert err[0] == 0, "an ASSERT of downsampleNormal fired"
    for im, theirs in zip(images, got):
        own = MO.stochastic(im, theirs.shape[1], theirs.shape[0])
        assert np.array_equal(own, theirs), im.shape


def test_coverage_bit_for_bit(ref):
    rng = np.random.default_rng(12)
    jobs, want = [], []
    for w, h in ((1, 1), (5, 3), (37, 21), (64, 64)):
        for kind in range(4):
            im = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
            if kind == 1:
                im[:, :, 3] = rng.choice([0, 255], (h, w))
            elif kind == 2:
                im[:, :, 3] = 0
            elif kind == 3:
                im[:, :, 3] = rng.integers(200, 256, (h, w))
            for ref_norm in (0.0, 0.25, 0.5, 1.0):
                jobs.append(("coverage", im, ref_norm, 0))
                want.append(MO.compute_coverage(im, ref_norm))
                for wanted in (0.0, 0.3, 0.5, 1.0, float(want[-1])):
                    jobs.append(("scale", im, ref_norm, wanted))
                    want.append(MO.scale_coverage(im, ref_norm, np.float32(wanted)))
    got, _ = ref_run(ref, jobs)
    infinite = 0
    for (op, im, a, b), theirs, own in zip(jobs, got, want):
        if op == "coverage":
            assert np.float32(own).tobytes() == np.float32(theirs).tobytes(), (im.shape, a)
        else:
            assert np.array_equal(own, theirs), (im.shape, a, b)
            with np.errstate(all="ignore"):
                infinite += bool(np.isinf(MO.coverage_scale(im, a, np.float32(b))))
    assert infinite > 0, "no case with new_ref == 0"


FILTER_SHAPES = ((64, 64), (64, 32), (33, 17), (32, 32), (17, 33), (16, 16), (8, 8), (7, 3), (5, 5), (4, 4), (3, 3), (2, 2), (1, 2), (2, 1))  # (w, h)


@pytest.mark.parametrize("mode,cap", [("linear", LINEAR_CAP), ("srgb", SRGB_CAP)])
def test_filtered_levels_within_1_of_stb(ref, mode, cap):
    rng = np.random.default_rng(13)
    images = []
    for w, h in FILTER_SHAPES:
        for k in range(40):
            im = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
            if k % 3 == 1:
                im[:, :, 3] = 255
            elif k % 3 == 2:
                im[:, :, 3] = np.where(rng.random((h, w)) < 0.75, 0, im[:, :, 3])
            images.append(im)
    got, times = ref_run(ref, [(mode, im, 0, 0) for im in images])
    n = differ = worst = 0
    for im, theirs in zip(images, got):
        a, b, c = shares(MO.compute_mip(im, theirs.shape[1], theirs.shape[0], OPS[mode]), theirs)
        n, differ, worst = n + a, differ + b, max(worst, c)
    ns, px = times[1 + 2 * OPS[mode]], times[2 + 2 * OPS[mode]]
    print(f"\n{mode}: {n} bytes compared, {differ} differ ({100.0 * differ / n:.4f} %), largest difference {worst}; the reference: {ns / max(px, 1):.1f} ns per output texel, one thread")
    assert worst <= 1, f"{mode}: a byte differs from stb's by {worst}"
    assert differ <= cap * n, f"{mode}: {differ} of {n} bytes differ, above the cap of {cap}"


def test_fixture_is_what_the_reference_gives(ref):
    g = np.load(GOLDEN)
    now = recorded(ref)
    assert sorted(g.files) == sorted(now)
    for k in g.files:
        assert np.array_equal(g[k], now[k]), k
    for mode, cap in (("linear", LINEAR_CAP), ("srgb", SRGB_CAP)):
        n, differ = g[f"share_{mode}"]
        print(f"\nfixture, {mode}: {differ} of {n} bytes differ from stb's ({100.0 * differ / n:.4f} %)")
        assert differ <= cap * n
