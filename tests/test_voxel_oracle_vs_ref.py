"""Pins tests/voxel_oracle.py to the reference's own code (CPU; skipped where the reference tree is absent).

At test time renderer/voxels.cpp - without voxelize(Model&) and forEachTriangle, which need the renderer's Model - and the core files it
calls (math.cpp, geometry.cpp) are copied into a temporary directory and compiled with g++ and the flags of tests/test_im_oracle_vs_ref.py;
core/stream.h is replaced there by the six members of OutputMemoryStream that Voxels calls on m_voxels (a byte vector), as the other
harnesses do, because stream.cpp pulls in the engine's allocators and locks. In the temporary copy of math.cpp the clock-seeded initialiser
of the thread-local generator is replaced by a fixed seed the harness can set and read. Nothing of the reference is committed; the harness only drives Voxels: voxelize's AABB loop over
the triangles (voxels.cpp:234-247, six lines of minimum / maximum) and bakeVertexAO's tail (model_importer.cpp:1346) are restated in it, and
the test asserts that the reference still holds those lines.

The oracle is held to the reference on every case of voxel_oracle.cases(): grid, voxel bytes, AO after every computeAO, the generator
behind it, the lookups, the blurred AO and the baked bytes, all bit for bit. This settles the argument order of
`Vec3(randFloat(), randFloat(), randFloat())`: g++ evaluates right to left, the first draw is z. tests/golden/make_golden_voxels.py records
tests/golden/voxels_small.npz with the same harness; the last test checks that the committed fixture is what the reference gives, and
prints the reference's single-thread time for the importer's shape (max_res 64, 32 rays)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import voxel_oracle as VO
from tests.test_im_oracle_vs_ref import FLAGS, REF, _block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxels_small.npz")

HARNESS = r"""
#include <cfloat>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "core/allocator.h"
#include "core/geometry.h"
#include "core/math.h"
#include "renderer/voxels.h"

namespace Lumix { void pin_seed(u32 u, u32 v); void pin_state(u32* out); }

struct Heap final : Lumix::IAllocator {
	void* allocate(size_t size, size_t align) override { return aligned_alloc(align < 16 ? 16 : align, (size + 15) / 16 * 16 + 16); }
	void deallocate(void* p) override { free(p); }
	void* reallocate(void* p, size_t n, size_t old, size_t align) override {
		void* q = allocate(n, align);
		if (p) { memcpy(q, p, old < n ? old : n); free(p); }
		return q;
	}
};

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) exit(2); return v; }

int main(int argc, char** argv) {
	using namespace Lumix;
	FILE* f = fopen(argv[1], "rb");
	FILE* o = fopen(argv[2], "wb");
	Heap heap;
	Voxels voxels(heap);
	const u32 use_begin = rd<u32>(f);
	Vec3 bmin = rd<Vec3>(f), bmax = rd<Vec3>(f);
	const u32 max_res = rd<u32>(f);
	const u32 n_meshes = rd<u32>(f);
	std::vector<std::vector<Vec3>> meshes(n_meshes);
	for (auto& m : meshes) {
		m.resize(3 * rd<u32>(f));
		if (!m.empty() && fread(m.data(), sizeof(Vec3), m.size(), f) != m.size()) return 2;
	}
	if (!use_begin) { // voxelize's AABB (voxels.cpp:234-247)
		Vec3 min = Vec3(FLT_MAX);
		Vec3 max = Vec3(-FLT_MAX);
		for (const auto& m : meshes)
			for (size_t t = 0; t < m.size(); t += 3) {
				min = minimum(min, m[t]);
				min = minimum(min, m[t + 1]);
				min = minimum(min, m[t + 2]);
				max = maximum(max, m[t]);
				max = maximum(max, m[t + 1]);
				max = maximum(max, m[t + 2]);
			}
		bmin = min; bmax = max;
	}
	voxels.beginRaster({bmin, bmax}, max_res);
	for (const auto& m : meshes)
		for (size_t t = 0; t < m.size(); t += 3) voxels.raster(m[t], m[t + 1], m[t + 2]);
	fwrite(&voxels.m_aabb.min, 4, 3, o);
	fwrite(&voxels.m_aabb.max, 4, 3, o);
	fwrite(&voxels.m_voxel_size, 4, 1, o);
	fwrite(&voxels.m_grid_resolution, 4, 3, o);
	const size_t n = (size_t)voxels.m_grid_resolution.x * voxels.m_grid_resolution.y * voxels.m_grid_resolution.z;
	fwrite(voxels.m_voxels.data(), 1, n, o);
	const u32 n_ao = rd<u32>(f);
	const u32 su = rd<u32>(f), sv = rd<u32>(f);
	pin_seed(su, sv);
	for (u32 k = 0; k < n_ao; ++k) {
		const u32 ray_count = rd<u32>(f);
		const auto t0 = std::chrono::steady_clock::now();
		voxels.computeAO(ray_count);
		if (argc > 3) fprintf(stderr, "computeAO %lld\n", (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
		fwrite(voxels.m_ao.begin(), 4, n, o);
		u32 state[2];
		pin_state(state);
		fwrite(state, 4, 2, o);
	}
	const u32 n_points = rd<u32>(f);
	std::vector<Vec3> points(n_points);
	if (n_points && fread(points.data(), sizeof(Vec3), n_points, f) != n_points) return 2;
	for (const Vec3& p : points) { u8 v = 0xEE; const u8 in = voxels.sample(p, &v) ? 1 : 0; fwrite(&v, 1, 1, o); fwrite(&in, 1, 1, o); }
	for (const Vec3& p : points) { float v = -7.f; voxels.sampleAO(p, &v); fwrite(&v, 4, 1, o); }
	const u32 n_bake = rd<u32>(f);
	std::vector<Vec3> verts(n_bake);
	if (n_bake && fread(verts.data(), sizeof(Vec3), n_bake, f) != n_bake) return 2;
	auto bake = [&]() {
		for (float min_ao : {0.f, 0.3f})
			for (const Vec3& p : verts) {
				float ao;
				u8 ao8 = 0xEE;
				if (voxels.sampleAO(p, &ao)) ao8 = u8(clamp((ao + min_ao) * 255, 0.f, 255.f) + 0.5f); // model_importer.cpp:1346
				fwrite(&ao8, 1, 1, o);
			}
	};
	bake();
	const auto t0 = std::chrono::steady_clock::now();
	voxels.blurAO();
	if (argc > 3) fprintf(stderr, "blurAO %lld\n", (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
	fwrite(voxels.m_ao.begin(), 4, n, o);
	bake();
	fclose(o);
	return 0;
}
"""

STREAM_H = r"""
#pragma once
#include <vector>
#include "core/allocator.h"
namespace Lumix {
struct OutputMemoryStream { // the members Voxels calls on m_voxels
	explicit OutputMemoryStream(IAllocator&) {}
	void resize(u64 n) { v.resize(n); }
	u8* getMutableData() { return v.data(); }
	const u8* data() const { return v.data(); }
	u64 size() const { return v.size(); }
	u8& operator[](u32 i) { return v[i]; }
	u8 operator[](u32 i) const { return v[i]; }
	std::vector<u8> v;
};
}
"""

SEED_HOOK = """static thread_local RandomGenerator rg(1, 1);
void pin_seed(u32 u, u32 v) { rg = RandomGenerator(u, v); }
void pin_state(u32* out) { memcpy(out, &rg, 8); }
"""


def build_harness(d):
    """compiles Voxels out of the reference into `d` (a directory outside the repository) -> the executable"""
    d = str(d)
    src = os.path.join(REF, "src")
    core = os.path.join(d, "core")
    shutil.copytree(os.path.join(src, "core"), core)
    sync = os.path.join(core, "sync.h")
    if os.path.exists(sync):
        open(sync, "w").write(open(sync).read().replace('#error "Not implemented"', "pthread_rwlock_t lock;", 1))
    # the generator: a fixed, settable seed instead of the clock
    math_cpp = open(os.path.join(core, "math.cpp")).read()
    seeded = "static thread_local RandomGenerator rg = initRandomGenerator();"
    assert seeded in math_cpp and "u = 36969 * (u & 65535) + (u >> 16);" in math_cpp and "return float(rand() * 2.328306435996595e-10);" in math_cpp
    open(os.path.join(core, "math.cpp"), "w").write("#include <string.h>\n" + math_cpp.replace(seeded, SEED_HOOK, 1))
    alt = os.path.join(d, "alt")  # in front of the include path of the two units that see Voxels
    os.makedirs(os.path.join(alt, "core"))
    open(os.path.join(alt, "core", "stream.h"), "w").write(STREAM_H)
    # Voxels without the two functions that need the renderer's Model
    os.makedirs(os.path.join(d, "renderer"))
    shutil.copy(os.path.join(src, "renderer", "voxels.h"), os.path.join(d, "renderer", "voxels.h"))
    vx = open(os.path.join(src, "renderer", "voxels.cpp")).read()
    for anchor in ("static void forEachTriangle(const Mesh& mesh, const F& f)", "void Voxels::voxelize(Model& model, u32 max_res)"):
        body = _block(vx, anchor)
        if "voxelize" in anchor:
            assert "min = minimum(min, p0);" in body and "max = maximum(max, p2);" in body and "Vec3 min = Vec3(FLT_MAX);" in body
        vx = vx.replace(anchor + " {" + body + "}", "", 1)
    vx = vx.replace("template <typename F>\n", "", 1).replace('#include "renderer/model.h"\n', "#include <string.h>\n", 1).replace('#include "core/profiler.h"\n', "", 1)
    assert "Model" not in vx and "forEachTriangle" not in vx
    assert "Vec3 dir = Vec3(randFloat(), randFloat(), randFloat()) * 2.f - 1.f;" in vx and "blurred[idx] = v / 9.f;" in vx
    open(os.path.join(d, "renderer", "voxels.cpp"), "w").write(vx)
    imp = open(os.path.join(src, "renderer", "editor", "model_importer.cpp")).read()
    assert "const u8 ao8 = u8(clamp((ao + min_ao) * 255, 0.f, 255.f) + 0.5f);" in imp and "voxels.computeAO(32);" in imp and "voxels.beginRaster(aabb, 64);" in imp
    open(os.path.join(d, "harness.cpp"), "w").write(HARNESS)
    stubs = os.path.join(d, "stubs.cpp")
    open(stubs, "w").write('#include "core/os.h"\nnamespace Lumix::os { u64 Timer::getRawTimestamp() { return 1; } }\n')
    inc = ["-I" + d, "-I" + src, "-I" + os.path.join(REF, "external")]
    units = [os.path.join(d, "harness.cpp"), stubs, os.path.join(d, "renderer", "voxels.cpp"), os.path.join(core, "math.cpp"), os.path.join(core, "geometry.cpp")]
    objs = []
    for path in units:
        obj = os.path.join(d, os.path.basename(path) + ".o")
        first = ["-I" + alt] if os.path.basename(path) in ("harness.cpp", "voxels.cpp") else []
        r = subprocess.run(["g++"] + FLAGS + first + inc + ["-c", path, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = os.path.join(d, "voxels_ref")
    r = subprocess.run(["g++"] + FLAGS + objs + ["-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_ref(ref, c, times=None):
    """a case of voxel_oracle.cases() through the reference -> the dict voxel_oracle.run_case gives (same keys, same points)"""
    exe, d = ref
    want = VO.run_case(c)  # (the lookup points derive from the grid; the comparison below does not depend on the oracle being right)
    u32 = lambda v: np.uint32(v).tobytes()
    begin = c["begin"] if c["begin"] is not None else ((0, 0, 0), (0, 0, 0))
    job = bytearray(u32(0 if c["begin"] is None else 1) + VO.f32(begin[0]).tobytes() + VO.f32(begin[1]).tobytes() + u32(c["max_res"]) + u32(len(c["meshes"])))
    for p, i in c["meshes"]:
        tris = np.ascontiguousarray(VO.mesh_triangles(p, i), np.float32)
        job += u32(len(tris)) + tris.tobytes()
    job += u32(len(c["ao"])) + u32(c["seed"][0]) + u32(c["seed"][1])
    for rc in c["ao"]:
        job += u32(rc)
    pts, verts = np.ascontiguousarray(want["points"], np.float32), np.ascontiguousarray(want["bake_vertices"], np.float32)
    job += u32(len(pts)) + pts.tobytes() + u32(len(verts)) + verts.tobytes()
    open(os.path.join(d, "job.bin"), "wb").write(bytes(job))
    r = subprocess.run([exe, os.path.join(d, "job.bin"), os.path.join(d, "out.bin")] + (["time"] if times is not None else []), check=True, timeout=300, capture_output=True, text=True)
    if times is not None:
        for line in r.stderr.split("\n"):
            if line.strip():
                kind, ns = line.split()
                times.setdefault(kind, []).append(int(ns))
    raw = open(os.path.join(d, "out.bin"), "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at).copy()
        at += a.nbytes
        return a

    g = dict(aabb_min=take("<f4", 3), aabb_max=take("<f4", 3), voxel_size=take("<f4", 1), resolution=take("<i4", 3))
    n = int(np.prod(g["resolution"].astype(np.int64)))
    g["voxels"] = take(np.uint8, n)
    for k in range(len(c["ao"])):
        g[f"ao{k}"] = take("<f4", n)
        g[f"rng{k}"] = take("<u4", 2)
    g["points"] = pts
    s = take(np.uint8, 2 * len(pts)).reshape(-1, 2)
    g["sample"], g["sample_inside"] = s[:, 0].copy(), s[:, 1].copy()
    g["sample_ao"] = take("<f4", len(pts))
    g["bake_vertices"] = verts
    g["bake_raw_0"], g["bake_raw_03"] = take(np.uint8, len(verts)), take(np.uint8, len(verts))
    g["blurred"] = take("<f4", n)
    g["bake_0"], g["bake_03"] = take(np.uint8, len(verts)), take(np.uint8, len(verts))
    assert at == len(raw)
    return g


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {k} {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(a.reshape(-1).view(np.uint8 if a.itemsize == 1 else np.uint32) != b.reshape(-1).view(np.uint8 if b.itemsize == 1 else np.uint32))[0]
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {a.size} places, first {bad[:5]}: {a.reshape(-1)[bad[:5]]} vs {b.reshape(-1)[bad[:5]]}")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.isdir(os.path.join(REF, "src")):
        pytest.skip("no reference tree on this machine")
    d = tmp_path_factory.mktemp("voxels_ref")
    return build_harness(d), str(d)


@pytest.mark.parametrize("name", list(VO.cases()))
def test_oracle_matches_the_reference(ref, name):
    c = VO.cases()[name]
    same(VO.run_case(c), run_ref(ref, c), name)


def test_draw_order_is_right_to_left(ref):
    """the reversed order (the first draw is x) does not give the reference's AO on any case with rays"""
    c = VO.cases()["cube"]
    got = run_ref(ref, c)
    assert VO.run_case(c, draw_order_reversed=True)["ao0"].tobytes() != got["ao0"].tobytes()
    assert VO.run_case(c)["ao0"].tobytes() == got["ao0"].tobytes()


def test_golden_fixture_is_what_the_reference_gives(ref):
    """tests/golden/voxels_small.npz (made by tests/golden/make_golden_voxels.py) still holds the reference's outputs of every case"""
    from tests.golden.make_golden_voxels import recorded

    g = np.load(GOLDEN)
    want = recorded(ref)
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        assert g[k].dtype == v.dtype and g[k].tobytes() == v.tobytes(), k


def test_reference_time_for_the_importers_shape(ref, capsys):
    """the CPU side of DESIGN.md §4.21: computeAO(32) and blurAO at max_res 64 on a sphere of 2000 triangles, single thread. A figure, no bar."""
    c = dict(meshes=[VO.sphere_mesh(26, 40)], max_res=64, begin=None, ao=[32], seed=(0xC0FFEE, 0xBADF00D))
    exe, d = ref
    # (run_ref would push 9.6 M rays through the numpy oracle first: the harness is driven directly, without lookups)
    u32 = lambda v: np.uint32(v).tobytes()
    tris = np.ascontiguousarray(VO.mesh_triangles(*c["meshes"][0]), np.float32)
    job = u32(0) + bytes(24) + u32(64) + u32(1) + u32(len(tris)) + tris.tobytes() + u32(1) + u32(c["seed"][0]) + u32(c["seed"][1]) + u32(32) + u32(0) + u32(0)
    open(os.path.join(d, "time.bin"), "wb").write(job)
    r = subprocess.run([exe, os.path.join(d, "time.bin"), os.path.join(d, "time_out.bin"), "time"], check=True, timeout=600, capture_output=True, text=True)
    times = dict((line.split()[0], int(line.split()[1])) for line in r.stderr.split("\n") if line.strip())
    res = np.frombuffer(open(os.path.join(d, "time_out.bin"), "rb").read(), "<i4", 3, 28)  # (behind the box and the voxel size)
    with capsys.disabled():
        print(f"\nreference, one thread, grid {res.tolist()}: computeAO(32) {times['computeAO'] / 1e6:.1f} ms, blurAO {times['blurAO'] / 1e6:.1f} ms")
    assert times["computeAO"] > 0
