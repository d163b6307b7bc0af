"""The host side of the voxel feature, without a device: lmx_voxels_rng_skip against sequential stepping, lmx_voxels_grid against the
oracle and the reference's record, the oracle against that record, and the mutant table - the oracle with one rule changed at a time must
disagree with the record on at least one case, or the cases are too tame to tell the rule."""
import os
import subprocess

import numpy as np
import pytest

from tests import voxel_oracle as VO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxels_small.npz")
OUTPUTS = ("aabb_min", "aabb_max", "voxel_size", "resolution", "voxels", "sample", "sample_inside", "sample_ao", "bake_raw_0", "bake_raw_03", "blurred", "bake_0", "bake_03")


# RandomGenerator::rand's two steps (core/math.cpp:1337-1341), one at a time: prints (u, v) behind each of the ascending draw counts given
STEPPER = r"""
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
	unsigned u = (unsigned)strtoul(argv[1], 0, 10), v = (unsigned)strtoul(argv[2], 0, 10);
	unsigned long long at = 0;
	for (int k = 3; k < argc; ++k) {
		const unsigned long long n = strtoull(argv[k], 0, 10);
		for (; at < n; ++at) {
			u = 36969u * (u & 65535u) + (u >> 16);
			v = 18000u * (v & 65535u) + (v >> 16);
		}
		printf("%u %u\n", u, v);
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def api():
    from lumixengine_amd import api as a
    from lumixengine_amd import build

    if not os.path.exists(a.LIB_PATH):
        build.build()
    return a


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def outputs_of(c):
    return OUTPUTS + tuple(f"{k}{n}" for n in range(len(c["ao"])) for k in ("ao", "rng"))


def test_rng_skip_matches_sequential_stepping(api, tmp_path):
    mu, mv = api.VOXEL_RNG_M_U, api.VOXEL_RNG_M_V
    rng = np.random.default_rng(11)
    halves = [1, 0xFFFFFFFF, 0x80000000, 0xFFFF, 0x10000, 65535 * 65536]
    us = halves + [mu - 1, mu, mu + 1] + [int(x) for x in rng.integers(1, 2 ** 32, 12)]
    vs = halves + [mv - 1, mv, mv + 1] + [int(x) for x in rng.integers(1, 2 ** 32, 12)]
    big = [2 ** 20 + 1, 3 * 32 * 300763]
    for u, v in zip(us, vs):
        state, at = (u, v), 0
        for n in (0, 1, 2, 3, 96):
            state, at = VO.rng_skip_sequential(state[0], state[1], n - at), n
            assert api.voxels_rng_skip(u, v, n) == state, (u, v, n)
    # the long jumps: one sequential walk per seed pair in a few lines of C (29 M steps each; Python would take minutes)
    src = tmp_path / "walk.c"
    src.write_text(STEPPER)
    exe = tmp_path / "walk"
    subprocess.run(["gcc", "-O2", "-std=c11", str(src), "-o", str(exe)], check=True)
    for k in range(len(us)):
        out = subprocess.run([str(exe), str(us[k]), str(vs[k])] + [str(n) for n in big], check=True, capture_output=True, text=True).stdout.split()
        for j, n in enumerate(big):
            assert api.voxels_rng_skip(us[k], vs[k], n) == (int(out[2 * j]), int(out[2 * j + 1])), (us[k], vs[k], n)
    # jumps compose: the state behind a + b draws is the state b draws behind the state behind a
    for a, b in ((5, 2 ** 40 + 3), (96, 3 * 65 * 2 ** 31)):
        mid = api.voxels_rng_skip(us[9], vs[9], a)
        assert api.voxels_rng_skip(mid[0], mid[1], b) == api.voxels_rng_skip(us[9], vs[9], a + b)
    assert api.voxels_rng_skip(0, 0, 1000) == (0, 0)  # (RandomGenerator asserts neither half is 0; compute_ao refuses them)


def test_grid_matches_oracle_and_reference(api, golden):
    for name, c in VO.cases().items():
        box = c["begin"]
        if box is None:  # voxelize's AABB, by the oracle
            o = VO.Voxels()
            tri = np.vstack([VO.mesh_triangles(p, i).reshape(-1, 3) for p, i in c["meshes"]])
            box = (tri.min(axis=0), tri.max(axis=0))
        g = api.voxels_grid(box[0], box[1], c["max_res"])
        mn, mx, vs, res = VO.grid(box[0], box[1], c["max_res"])
        for got, want, key in ((g["aabb_min"], mn, "aabb_min"), (g["aabb_max"], mx, "aabb_max"), (g["voxel_size"], vs, "voxel_size"), (g["resolution"], res.astype(np.int32), "resolution")):
            assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (name, key)
            assert np.asarray(got).tobytes() == golden[f"{name}|{key}"].tobytes(), (name, key)
    # a flat mesh: the thin axis is 3 * vs / vs, whatever fp32 makes of it
    assert golden["flat quad|resolution"].tolist()[2] in (2, 3)
    rng = np.random.default_rng(2)
    for _ in range(300):
        lo = rng.uniform(-100, 100, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 30, 3).astype(np.float32) * (rng.random(3) > 0.2)).astype(np.float32)
        if not (hi > lo).any():
            continue
        res = int(rng.integers(1, 200))
        g = api.voxels_grid(lo, hi, res)
        mn, mx, vs, r = VO.grid(lo, hi, res)
        assert g["aabb_min"].tobytes() == mn.tobytes() and g["aabb_max"].tobytes() == mx.tobytes() and g["voxel_size"].tobytes() == vs.tobytes()
        assert g["resolution"].tolist() == r.tolist()


def test_grid_refusals(api):
    for args in (((0, 0, 0), (1, 1, 1), 0), ((0, 0, 0), (np.nan, 1, 1), 4), ((0, -np.inf, 0), (1, 1, 1), 4), ((0, 0, 0), (0, 0, 0), 4), ((1, 1, 1), (0, 0, 0), 4),
                 ((0, 0, 0), (1, 1, 1), 1300), ((0, 0, 0), (3e38, 3e38, 3e38), 4)):
        with pytest.raises(api.LumixError) as e:
            api.voxels_grid(*args)
        assert e.value.code == 1, args
    big = api.voxels_grid((0, 0, 0), (1, 1, 1), 1280)["resolution"].tolist()  # 2.1e9 cells: accepted
    assert big == VO.grid((0, 0, 0), (1, 1, 1), 1280)[3].tolist() and 2 ** 30 < big[0] * big[1] * big[2] < 2 ** 31


@pytest.mark.parametrize("name", list(VO.cases()))
def test_oracle_matches_the_record(golden, name):
    c = VO.cases()[name]
    r = VO.run_case(c)
    for k in outputs_of(c):
        assert r[k].dtype == golden[f"{name}|{k}"].dtype and r[k].tobytes() == golden[f"{name}|{k}"].tobytes(), k
    # the record's inputs are the cases'
    for m, (p, i) in enumerate(c["meshes"]):
        assert golden[f"{name}|positions{m}"].tobytes() == np.ascontiguousarray(p, np.float32).tobytes() and golden[f"{name}|indices{m}"].tobytes() == np.ascontiguousarray(i).tobytes()
    assert golden[f"{name}|seed"].tolist() == list(c["seed"]) and golden[f"{name}|ray_counts"].tolist() == list(c["ao"]) and r["points"].tobytes() == golden[f"{name}|points"].tobytes()


@pytest.mark.parametrize("rule", VO.RULES)
def test_mutant_disagrees_with_the_record(golden, rule):
    """draw order reversed; true division for the reciprocal multiply in `dir /=` and to_grid; floor for truncation; one `p += dir`; >= for >
    in the march's bounds; / 27; 1 - k * inv; the AABB over all vertices"""
    killed = []
    for name, c in VO.cases().items():
        r = VO.run_case(c, **{rule: True})
        if any(r[k].tobytes() != golden[f"{name}|{k}"].tobytes() for k in outputs_of(c)):
            killed.append(name)
    assert killed, f"the mutant `{rule}` gives the reference's outputs on every case: the cases are too tame"


def test_host_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """csrc/lmx_voxels.h as host code - grid, cell boxes, the box/triangle test, the skip, the march, lookups, the bake - at its edges in a
    stand-alone program (tests/cpp/voxels_host_sanitize.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "voxels_host_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "lumixengine_amd", "csrc"), os.path.join(root, "tests", "cpp", "voxels_host_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
