"""Pins tests/ray_scene_oracle.py to the reference's own code (CPU; skipped where the reference tree is absent).

At test time the body of RenderModuleImpl::castRayProceduralGeometry and the tail of castRay (renderer/render_module.cpp, from the
procedural-geometry call to the end of the terrain loop) and, out of renderer/terrain.cpp, the bodies of Terrain::castRay and of both
Terrain::getHeight are cut out of the reference tree into a temporary directory and compiled with -msse2 -mfpmath=sse -ffp-contract=off
against the real core headers, with core/math.cpp and core/geometry.cpp compiled in place, the way tests/test_ray_oracle_vs_ref.py does
it for the model-instance loop. Nothing of the reference is committed: the harness only declares the containers the slices read (a
procedural geometry and the map of them, a texture, a terrain's members, the world's transforms, the hit record and the `ignored` filter).
The hit castRay holds when it reaches the tail comes from ray_oracle / ray_im_oracle, which are pinned by their own tests. The
reference's records - per ray the procedural hit (is_hit, entity, t), per (ray, terrain) the terrain hit (is_hit, t), per ray the merged
hit (is_hit, component, entity, t) - must equal the oracle's bit for bit on the scenes of tests/test_gpu_rays_scene.py.

Every ray the binary is given must end its terrain walks (ray_scene_oracle's walk_ends): asserted before the binary starts, which runs
under a timeout. The zero-step rays are held to the oracle by the device tests only. tests/golden/make_golden_rays_scene.py records one
scene's hits with the same harness."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from lumixengine_amd import api
from tests import ray_scene_oracle as RSO
from tests import test_gpu_rays_scene as S
from tests.test_im_oracle_vs_ref import FLAGS, REF, _block

HARNESS = r"""
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <math.h>
#include <vector>
#include "core/geometry.h"
#include "core/math.h"
#include "engine/lumix.h"

namespace pin {
using namespace Lumix;

namespace gpu {
enum class PrimitiveType : u32 { TRIANGLES, TRIANGLE_STRIP, LINES, POINTS, NONE };
enum class DataType : u32 { U16, U32 };
enum class TextureFormat : u32 { R16, RGBA8 };
}
template <typename T> struct Arr { // the members of Array<T> / OutputMemoryStream the slices call
	std::vector<T> v;
	bool empty() const { return v.empty(); }
	size_t size() const { return v.size(); }
	const T* data() const { return v.data(); }
};
struct Mesh;
struct RayCastModelHit;
struct Filter { EntityPtr ignored; bool invoke(const RayCastModelHit& hit) const; };
struct RayCastModelHit {
	bool is_hit;
	float t;
	DVec3 origin;
	Vec3 dir;
	Mesh* mesh;
	EntityPtr entity;
	int component_type;
	u32 subindex;
	using Filter = pin::Filter;
};
bool Filter::invoke(const RayCastModelHit& hit) const { return hit.entity != ignored || !ignored.isValid(); } // :2603-2607
namespace types { static const int procedural_geom = 11; static const int terrain = 12; }
struct VertexDecl {
	gpu::PrimitiveType primitive_type = gpu::PrimitiveType::TRIANGLES;
	u32 stride = 0;
	u32 getStride() const { return stride; }
};
struct ProceduralGeometry {
	Arr<u8> vertex_data;
	Arr<u8> index_data;
	VertexDecl vertex_decl;
	gpu::DataType index_type = gpu::DataType::U16;
	AABB aabb;
	u32 index_count = 0;
	u32 getIndexCount() const { return index_count; }
};
struct PgItem {
	EntityRef e;
	const ProceduralGeometry* pg;
	EntityRef key() const { return e; }
	const ProceduralGeometry& value() const { return *pg; }
};
struct PgMap {
	std::vector<PgItem> items;
	const std::vector<PgItem>& iterated() const { return items; }
};
struct World {
	std::vector<Transform> tr;
	const Transform& getTransform(EntityRef e) const { return tr[e.index]; }
	DVec3 getPosition(EntityRef e) const { return tr[e.index].pos; }
};
struct Texture {
	gpu::TextureFormat format;
	std::vector<u8> bytes;
	bool ready = true;
	const u8* getData() const { return bytes.data(); }
	bool isReady() const { return ready; }
};
struct Module;
struct Terrain {
	Texture* m_heightmap = nullptr;
	i32 m_width = 0, m_height = 0;
	Vec3 m_scale;
	EntityRef m_entity;
	Module& m_module;
	explicit Terrain(Module& m) : m_module(m) {}
	EntityRef getEntity() const { return m_entity; }
	float getHeight(float x, float z) const;
	float getHeight(int x, int z) const;
	RayCastModelHit castRay(const Ray& ray);
};
struct Module {
	World m_world;
	PgMap m_procedural_geometries;
	std::vector<Terrain*> m_terrains;
	const World& getWorld() const { return m_world; }
	RayCastModelHit castRayProceduralGeometry(const Ray& ray, const RayCastModelHit::Filter& filter) {
#include "module_cast_ray_pg.inc"
	}
	// `hit`: what castRay holds when the model-instance loop is done (:2759)
	RayCastModelHit castRayTail(const Ray& ray, const Filter& filter, RayCastModelHit hit) {
#include "module_cast_ray_tail.inc"
		return hit;
	}
};
float Terrain::getHeight(float x, float z) const {
#include "terrain_height_f.inc"
}
float Terrain::getHeight(int x, int z) const {
#include "terrain_height_i.inc"
}
RayCastModelHit Terrain::castRay(const Ray& ray) {
#include "terrain_cast_ray.inc"
}
} // namespace pin

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) exit(2); return v; }

int main(int argc, char** argv) {
	using namespace Lumix;
	FILE* f = fopen(argv[1], "rb");
	FILE* o = fopen(argv[2], "wb");
	pin::Module module;
	module.m_world.tr.resize(rd<u32>(f));
	for (Transform& t : module.m_world.tr)
		if (fread(&t.pos, 8, 3, f) != 3 || fread(&t.rot, 4, 4, f) != 4 || fread(&t.scale, 4, 3, f) != 3) return 2;
	std::vector<pin::ProceduralGeometry> pgs(rd<u32>(f));
	for (pin::ProceduralGeometry& pg : pgs) {
		const i32 entity = rd<i32>(f);
		pg.vertex_decl.primitive_type = rd<u32>(f) ? pin::gpu::PrimitiveType::TRIANGLES : pin::gpu::PrimitiveType::LINES;
		float box[6];
		if (fread(box, 4, 6, f) != 6) return 2;
		pg.aabb.min = Vec3(box[0], box[1], box[2]); pg.aabb.max = Vec3(box[3], box[4], box[5]);
		pg.vertex_decl.stride = rd<u32>(f);
		pg.vertex_data.v.resize(rd<u32>(f));
		if (!pg.vertex_data.v.empty() && fread(pg.vertex_data.v.data(), 1, pg.vertex_data.v.size(), f) != pg.vertex_data.v.size()) return 2;
		pg.index_type = rd<u32>(f) == 2 ? pin::gpu::DataType::U16 : pin::gpu::DataType::U32;
		pg.index_count = rd<u32>(f);
		pg.index_data.v.resize(rd<u32>(f));
		if (!pg.index_data.v.empty() && fread(pg.index_data.v.data(), 1, pg.index_data.v.size(), f) != pg.index_data.v.size()) return 2;
		module.m_procedural_geometries.items.push_back(pin::PgItem{EntityRef{entity}, &pg});
	}
	const u32 nt = rd<u32>(f);
	std::vector<pin::Texture> textures(nt);
	std::vector<pin::Terrain> terrains(nt, pin::Terrain(module));
	for (u32 k = 0; k < nt; ++k) {
		pin::Terrain& t = terrains[k];
		t.m_entity = EntityRef{rd<i32>(f)};
		t.m_width = rd<i32>(f); t.m_height = rd<i32>(f);
		if (fread(&t.m_scale, 4, 3, f) != 3) return 2;
		textures[k].format = rd<u32>(f) == 0 ? pin::gpu::TextureFormat::R16 : pin::gpu::TextureFormat::RGBA8;
		textures[k].ready = rd<u32>(f) != 0;
		textures[k].bytes.resize(rd<u32>(f));
		if (!textures[k].bytes.empty() && fread(textures[k].bytes.data(), 1, textures[k].bytes.size(), f) != textures[k].bytes.size()) return 2;
		t.m_heightmap = &textures[k];
		module.m_terrains.push_back(&t);
	}
	const u32 nr = rd<u32>(f);
	for (u32 r = 0; r < nr; ++r) {
		Ray ray;
		if (fread(&ray.origin, 8, 3, f) != 3 || fread(&ray.dir, 4, 3, f) != 3) return 2;
		rd<float>(f); // (t_max: castRay(ray, ignored) knows none; the caller's `held` is applied by the test)
		pin::Filter filter;
		filter.ignored = EntityPtr{rd<i32>(f)};
		rd<u32>(f);
		pin::RayCastModelHit held; // the hit of the stages before, from their own pinned oracles
		memset(&held, 0, sizeof(held));
		held.is_hit = rd<u32>(f) != 0;
		held.component_type = (int)rd<u32>(f);
		held.entity = EntityPtr{rd<i32>(f)};
		held.t = rd<float>(f);
		const pin::RayCastModelHit pg = module.castRayProceduralGeometry(ray, filter);
		u32 out[3] = {pg.is_hit ? 1u : 0u, pg.is_hit ? (u32)pg.entity.index : 0u, 0u};
		float t = pg.is_hit ? pg.t : 0;
		memcpy(&out[2], &t, 4);
		fwrite(out, 4, 3, o);
		for (pin::Terrain* te : module.m_terrains) {
			const pin::RayCastModelHit th = te->castRay(ray);
			u32 rec[2] = {th.is_hit ? 1u : 0u, 0u};
			t = th.is_hit ? th.t : 0;
			memcpy(&rec[1], &t, 4);
			fwrite(rec, 4, 2, o);
		}
		const pin::RayCastModelHit hit = module.castRayTail(ray, filter, held);
		u32 fin[4] = {hit.is_hit ? 1u : 0u, hit.is_hit ? (u32)hit.component_type : 0u, hit.is_hit ? (u32)hit.entity.index : 0u, 0u};
		t = hit.is_hit ? hit.t : 0;
		memcpy(&fin[3], &t, 4);
		fwrite(fin, 4, 4, o);
	}
	fclose(o);
	return 0;
}
"""

COMPONENT = {RSO.MODEL_INSTANCE: 7, RSO.INSTANCED_MODEL: 9, RSO.PROCEDURAL_GEOM: 11, RSO.TERRAIN: 12}  # the harness' types::


def slice_reference(out):
    src = os.path.join(REF, "src")
    rm = open(os.path.join(src, "renderer", "render_module.cpp")).read()
    pg = _block(rm, "RayCastModelHit castRayProceduralGeometry(const Ray& ray, const RayCastModelHit::Filter& filter) {")
    assert "tr.invTransformVector(ray.dir)" in pg and "pg.aabb.contains(ro)" in pg and "getRayTriangleIntersection(ro, rd, a, b, c, &t)" in pg and "return hit;" in pg
    body = _block(rm, "RayCastModelHit castRay(const Ray& ray, const Delegate<bool (const RayCastModelHit&)> filter) override {")
    tail = body[body.index("const RayCastModelHit pg_hit"):body.index("hit.origin = ray.origin;", body.index("for (auto* terrain : m_terrains)"))]
    assert "pg_hit.t < hit.t || !hit.is_hit" in tail and "terrain->castRay(ray)" in tail and "filter.invoke(terrain_hit)" in tail
    te = open(os.path.join(src, "renderer", "terrain.cpp")).read()
    cast = _block(te, "RayCastModelHit Terrain::castRay(const Ray& ray)")
    assert "m_scale.z / fabsf(ray.dir.z)" in cast and "next_x < next_z && step_x != 0" in cast and "delta_x == 0 && delta_z == 0" in cast
    hf = _block(te, "float Terrain::getHeight(float x, float z) const")
    assert "dec_x > dec_z" in hf and "inv_scale" in hf
    hi = _block(te, "float Terrain::getHeight(int x, int z) const")
    assert "DIV64K" in hi and "clamp(x, 0, m_width - 1)" in hi
    for name, text in (("module_cast_ray_pg.inc", pg), ("module_cast_ray_tail.inc", tail), ("terrain_cast_ray.inc", cast), ("terrain_height_f.inc", hf), ("terrain_height_i.inc", hi)):
        open(os.path.join(out, name), "w").write(text + "\n")


def build_harness(d):
    """compiles the sliced reference into `d` (a directory outside the repository) -> the executable"""
    d = str(d)
    core = os.path.join(d, "core")
    shutil.copytree(os.path.join(REF, "src", "core"), core)  # (core/sync.h, as in tests/test_ray_oracle_vs_ref.py)
    sync = os.path.join(core, "sync.h")
    if os.path.exists(sync):
        open(sync, "w").write(open(sync).read().replace('#error "Not implemented"', "pthread_rwlock_t lock;", 1))
    gen = os.path.join(d, "gen")
    os.makedirs(gen)
    slice_reference(gen)
    open(os.path.join(d, "harness.cpp"), "w").write(HARNESS)
    inc = ["-I" + d, "-I" + gen, "-I" + os.path.join(REF, "src"), "-I" + os.path.join(REF, "external")]
    objs = []
    for path in (os.path.join(d, "harness.cpp"), os.path.join(REF, "src", "core", "math.cpp"), os.path.join(REF, "src", "core", "geometry.cpp")):
        obj = os.path.join(d, os.path.basename(path) + ".o")
        r = subprocess.run(["g++"] + FLAGS + inc + ["-c", path, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = os.path.join(d, "ray_scene_ref")
    stubs = os.path.join(d, "stubs.cpp")
    open(stubs, "w").write('#include "core/os.h"\nnamespace Lumix::os { u64 Timer::getRawTimestamp() { return 1; } }\n')
    r = subprocess.run(["g++"] + FLAGS + inc + [stubs] + objs + ["-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def held_hits(want):
    """the hit castRay holds behind the model-instance loop (:2759), from the earlier stages' oracles: (is_hit, component, entity, t)"""
    n = len(want["hits"])
    held = np.zeros(n, np.dtype([("is_hit", "<u4"), ("component", "<u4"), ("entity", "<i4"), ("t", "<f4")]))
    for r in range(n):
        if want["hits"][r]["is_hit"]:
            held[r] = (1, COMPONENT[RSO.MODEL_INSTANCE], want["hits"][r]["entity"], want["hits"][r]["t"])
        elif want["im"] is not None and want["im"][r]["is_hit"]:
            held[r] = (1, COMPONENT[RSO.INSTANCED_MODEL], want["im"][r]["entity"], want["im"][r]["t"])
    return held


def run_ref(exe, d, sc, rays, held):
    """-> the reference's (procedural hits, terrain hits [ray, terrain], merged hits) with the fields it does not keep left zero"""
    u32 = lambda v: np.uint32(v).tobytes()
    n_ent = 1 + max([len(sc["transforms"]) - 1] + [int(g["entity"]) for g in sc["pg"]] + [int(t["entity"]) for t in sc["terrains"]])
    tr = np.zeros(n_ent, api.TRANSFORM)
    tr[: len(sc["transforms"])] = sc["transforms"]
    job = bytearray(u32(n_ent))
    for t in tr:
        job += t["pos"].astype(np.float64).tobytes() + t["rot"].astype(np.float32).tobytes() + t["scale"].astype(np.float32).tobytes()
    job += u32(len(sc["pg"]))
    for g in sc["pg"]:
        v = np.frombuffer(np.ascontiguousarray(g["vertex_data"]).tobytes(), np.uint8)
        idx = g.get("indices")
        i = np.zeros(0, np.uint32) if idx is None else np.ascontiguousarray(idx).reshape(-1)
        job += np.int32(g["entity"]).tobytes() + u32(1 if g.get("triangles", True) else 0) + np.asarray(g["aabb_min"], np.float32).tobytes() + np.asarray(g["aabb_max"], np.float32).tobytes()
        job += u32(g["stride"]) + u32(len(v)) + v.tobytes() + u32(i.dtype.itemsize) + u32(g.get("index_count", len(i))) + u32(i.nbytes) + i.tobytes()
    job += u32(len(sc["terrains"]))
    for t in sc["terrains"]:
        h = np.ascontiguousarray(t["heightmap"])
        job += np.int32(t["entity"]).tobytes() + np.int32(h.shape[1]).tobytes() + np.int32(h.shape[0]).tobytes() + np.asarray(t["scale"], np.float32).tobytes()
        job += u32(0 if h.dtype == np.uint16 else 1) + u32(1 if t.get("ready", True) else 0) + u32(h.nbytes) + h.tobytes()
    rays = np.ascontiguousarray(rays, api.RAY)
    job += u32(len(rays))
    for r in range(len(rays)):
        job += rays[r : r + 1].tobytes() + held[r : r + 1].tobytes()
    open(os.path.join(d, "job.bin"), "wb").write(bytes(job))
    subprocess.run([exe, os.path.join(d, "job.bin"), os.path.join(d, "out.bin")], check=True, timeout=120)
    nt = len(sc["terrains"])
    rec = np.dtype([("pg", [("is_hit", "<u4"), ("entity", "<i4"), ("t", "<f4")]), ("terrain", [("is_hit", "<u4"), ("t", "<f4")], (nt,)),
                    ("scene", [("is_hit", "<u4"), ("component", "<u4"), ("entity", "<i4"), ("t", "<f4")])])
    raw = np.frombuffer(open(os.path.join(d, "out.bin"), "rb").read(), rec, len(rays))
    return raw["pg"], raw["terrain"].reshape(len(rays), nt), raw["scene"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.isdir(os.path.join(REF, "src")):
        pytest.skip("no reference tree on this machine")
    d = tmp_path_factory.mktemp("ray_scene_ref")
    return build_harness(d), str(d)


def reference_records(ref, sc, rays):
    """-> (the oracle's records, the reference's) for rays without a t_max: castRay(ray, ignored) has none"""
    rays = np.array(rays, copy=True)
    rays["t_max"] = np.inf
    want = RSO.cast_scene(sc, rays)
    assert want["walk_ends"].all(), "a ray whose terrain walk the reference never ends must not reach the binary"
    assert RSO.agrees(sc, rays), "a bad scene: the reference's walk and the order-free form differ (a NaN t)"
    return want, run_ref(ref[0], ref[1], sc, rays, held_hits(want))


def pinned(ref, scene, what):
    sc, rays = scene
    want, (pg, th, fin) = reference_records(ref, sc, rays)
    for k in ("is_hit", "entity", "t"):
        assert pg[k].tobytes() == want["pg"][k].astype(pg[k].dtype).tobytes(), f"{what}: procedural {k}: reference {pg[k]} vs oracle {want['pg'][k]}"
    for k in ("is_hit", "t"):
        assert th[k].tobytes() == want["terrain"][k].astype(th[k].dtype).tobytes(), f"{what}: terrain {k}: reference {th[k]} vs oracle {want['terrain'][k]}"
    comp = np.array([COMPONENT.get(int(c), 0) for c in want["scene"]["component"]], np.uint32)
    for k, mine in (("is_hit", want["scene"]["is_hit"]), ("component", comp), ("entity", want["scene"]["entity"]), ("t", want["scene"]["t"])):
        assert fin[k].tobytes() == mine.astype(fin[k].dtype).tobytes(), f"{what}: castRay {k}: reference {fin[k]} vs oracle {mine}"
    return want


def ending(scene):
    """the scene's rays whose terrain walks end: dir.x != 0 && dir.z != 0 (magnitudes below 0.01 included) or the vertical ray"""
    sc, rays = scene
    d = rays["dir"]
    return sc, rays[((d[:, 0] != 0) & (d[:, 2] != 0)) | ((d[:, 0] == 0) & (d[:, 2] == 0))]


def test_procedural_scenes_match_the_reference(ref):
    assert pinned(ref, S.single_triangle_scene(), "single triangle")["pg"]["is_hit"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0]
    assert pinned(ref, S.contains_scene(), "contains")["pg"]["is_hit"].tolist() == [1, 0, 1]
    assert pinned(ref, S.skips_scene(), "skips")["pg"]["entity"].tolist() == [2, 3, 2, 2]
    assert pinned(ref, S.twins_scene(), "twins")["pg"]["entity"].tolist() == [0, 1, 2]
    sc, rays = S.mixed_scene()
    assert pinned(ref, (sc, rays), "mixed")["pg"]["is_hit"].sum() >= 8


@pytest.mark.parametrize("shape", [(8, 8), (70, 3), (3, 70), (130, 130)])
def test_terrain_maps_match_the_reference(ref, shape):
    for dtype in (np.uint16, np.uint32):
        for scale_z in (1.5, 2.25):
            want = pinned(ref, ending(S.map_scene(*shape, dtype, scale_z)), f"{shape} {np.dtype(dtype).name} scale.z {scale_z}")
            assert want["terrain"]["is_hit"].sum() >= 4


def test_terrain_walk_cases_match_the_reference(ref):
    w = 130
    flat = S.bare(S.transforms([[0, 0, 0]]), [], [S.terrain(0, np.zeros((w, w), np.uint16), np.float32([1, 20.0, 1]))])
    assert pinned(ref, (flat, S.flat_walk_rays(w, 1.0, 1.0)), "chunk edges")["terrain"]["is_hit"].all()
    assert pinned(ref, ending(S.saddle_scene()), "saddle")["terrain"]["is_hit"].all()
    assert pinned(ref, ending(S.origins_scene()), "origins")["terrain"]["is_hit"][:, 0].tolist() == [1, 1, 1, 0, 1, 0]
    sc, rays = S.threshold_scene()
    assert len(ending((sc, rays))[1]) == len(rays)
    assert pinned(ref, (sc, rays), "0.01")["terrain"]["is_hit"].sum() >= 12


def test_merge_matches_the_reference(ref):
    """the mixed scene with model-instance hits ahead of the tail; ignore names a geometry's and a terrain's entity"""
    sc, rays = S.mixed_scene(100)
    want = pinned(ref, (sc, rays), "merge")
    assert {RSO.MODEL_INSTANCE, RSO.PROCEDURAL_GEOM, RSO.TERRAIN} <= set(want["scene"]["component"].tolist())


def test_golden_fixture_is_what_the_reference_gives(ref):
    """tests/golden/rays_scene_small.npz (made by tests/golden/make_golden_rays_scene.py) still holds the reference's records for golden_scene()"""
    g = np.load(os.path.join(S.GOLDEN, "rays_scene_small.npz"))
    sc, rays = S.golden_scene()
    assert g["rays"].tobytes() == rays.tobytes()
    want, (pg, th, fin) = reference_records(ref, sc, rays)
    from tests.golden.make_golden_rays_scene import recorded

    for k, v in recorded(sc, rays, pg, th, fin).items():
        assert g[k].tobytes() == v.tobytes(), k
