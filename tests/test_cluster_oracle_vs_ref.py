"""Pins tests/cluster_oracle.py and lmx_clusters_planes to the reference's own code (CPU; skipped where the reference tree is absent).

At test time these parts of the brace-matched body of PipelineImpl::fillClusters (renderer/pipeline.cpp) are cut out of the reference tree
into a temporary directory by text anchors, the way tests/test_im_oracle_vs_ref.py cuts encodeInstancedModels, and compiled with
-msse2 -mfpmath=sse -ffp-contract=off against the real headers (Vec3 / Vec4 / DVec3 / Quat, ShiftedFrustum, makePlane, planeDist,
core/sort.h, PointLight / EnvironmentProbe / ReflectionProbe of renderer/render_module.h) with core/math.cpp and core/geometry.cpp
compiled in place:

  cl_structs.inc   the four local structs ClusterLight, Cluster, ClusterEnvProbe, ClusterReflProbe
  cl_size.inc      the `size` statement (the cluster grid of the viewport)
  cl_clusters.inc  `clusters_count`, the allocation of `clusters` and its memset
  cl_cam.inc       the `cam_pos` statement
  cl_light.inc     the body of the light list's forEach from its `pl` and `light` references through attenuation_param: the record
                   statements that do not touch the shadow atlas (radius, Vec3(light_pos - cam_pos), rot, fov, color * intensity,
                   attenuation_param)
  cl_planes.inc    the probe spans, the allocation of `env_probes` and `refl_probes` and the `frustum` reference in front of
                   `Vec4 xplanes[65];`, then the plane block through the x-plane loop
  cl_probes.inc    the two probe record loops with their sort calls
  cl_range.inc     the `range` lambda
  cl_binning.inc   `auto for_each_light_pair` through the loop that takes the counts back off cluster.offset: the three count passes, the
                   prefix, the map allocation, the three fill passes and the restore

Nothing of the reference is committed. The harness below declares what the slices read and does file I/O; none of its stand-ins computes
anything:

  World            getPosition / getRotation return the fields of the harness's transform table
  Module           getPointLight returns the record of an entity; getReflectionProbes / getEnvironmentProbes /
                   getReflectionProbesEntities / getEnvironmentProbesEntities return Spans over the harness's arrays of the real types
  FrameAllocator   allocate(size, align): zeroed memory (the reference's arena leaves it as it was; so the recorded fixture's padding
                   words, which no slice writes, are zero as the library's are)
  m_viewport       w and h of the job file; cp: pos and frustum of the job file
  lights,          zeroed room for one record per listed entity and the list's length, from the job file (the reference sizes them from
  lights_count     the cull result); atlas_idx, which no slice writes, is not compared
  the loop over the listed entities around cl_light.inc (CullResult::forEach in the reference), and the loop that calls range() for the
  job's spheres

What this does NOT pin - DESIGN.md 4.11's deviations: the library and the oracle take enabled probes only and keep ties in module order.
The reference sorts the records of disabled probes without having initialised them, and its sort makes no promise about ties, so every
probe here is enabled and the volume products are pairwise distinct (tests/test_gpu_clusters.py::test_probes_order_and_segments keeps
covering our own rule). The shadow-atlas slot of a light record is a table here (deviation 3) and is left out too."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from lumixengine_amd import api
from tests import cluster_oracle as CO

REF = "/root/reference"
FP = ["-O2", "-msse2", "-mfpmath=sse", "-ffp-contract=off", "-fno-fast-math"]
FLAGS = ["-std=c++20", "-fno-exceptions", "-fno-rtti", "-DSTATIC_PLUGINS", "-DNDEBUG", "-Wno-multichar", "-w"] + FP

HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "core/core.h"
#include "core/geometry.h"
#include "core/math.h"
#include "core/os.h"
#include "core/sort.h"
#include "core/span.h"
#include "engine/lumix.h"
#include "renderer/render_module.h"

namespace pin {
using namespace Lumix;

#include "cl_structs.inc"
static_assert(sizeof(ClusterLight) == 64 && sizeof(Cluster) == 16 && sizeof(ClusterEnvProbe) == 208 && sizeof(ClusterReflProbe) == 48, "records");
static_assert(sizeof(Transform) == 56 && sizeof(ShiftedFrustum) == 256 && sizeof(EnvironmentProbe) == 136 && sizeof(EntityRef) == 4, "inputs");

struct World {
	const Transform* tr;
	DVec3 getPosition(EntityRef e) const { return tr[e.index].pos; }
	Quat getRotation(EntityRef e) const { return tr[e.index].rot; }
};

struct Module {
	PointLight* point_lights;
	Span<const ReflectionProbe> refl;
	Span<const EnvironmentProbe> env;
	Span<EntityRef> refl_entities, env_entities;
	PointLight& getPointLight(EntityRef e) { return point_lights[e.index]; }
	Span<const ReflectionProbe> getReflectionProbes() { return refl; }
	Span<const EnvironmentProbe> getEnvironmentProbes() { return env; }
	Span<EntityRef> getReflectionProbesEntities() { return refl_entities; }
	Span<EntityRef> getEnvironmentProbesEntities() { return env_entities; }
};

struct FrameAllocator {
	void* allocate(size_t size, size_t align) { return calloc(size / 16 + 2, 16); }
};

struct CameraParams { DVec3 pos; ShiftedFrustum frustum; };
struct ViewportSize { int w, h; };
struct Sphere { Vec3 p; float r; };

// `lights`: zeroed room for one record per listed entity, the harness's own
void run(Module* m_module, const World& world, FrameAllocator& frame_allocator, const CameraParams& cp, const ViewportSize& m_viewport, const std::vector<EntityRef>& listed,
         const i32 lights_count, ClusterLight* lights, const std::vector<Sphere>& spheres, FILE* o) {
#include "cl_size.inc"
#include "cl_clusters.inc"
#include "cl_cam.inc"
	for (i32 i = 0; i < lights_count; ++i) {
		const EntityRef e = listed[i];
#include "cl_light.inc"
	}
#include "cl_planes.inc"
#include "cl_probes.inc"
#include "cl_range.inc"
#include "cl_binning.inc"
	fwrite(&size, 4, 3, o);
	fwrite(xplanes, 16, size.x + 1, o);
	fwrite(yplanes, 16, size.y + 1, o);
	fwrite(zplanes, 16, size.z + 1, o);
	fwrite(lights, sizeof(ClusterLight), lights_count, o);
	fwrite(env_probes, sizeof(ClusterEnvProbe), module_env_probes.length(), o);
	fwrite(refl_probes, sizeof(ClusterReflProbe), module_refl_probes.length(), o);
	fwrite(clusters, sizeof(Cluster), clusters_count, o);
	fwrite(&offset, 4, 1, o);
	fwrite(map, 4, offset, o);
	for (const Sphere& s : spheres) {
		const IVec2 r[3] = {range(s.p, s.r, size.x, xplanes), range(s.p, s.r, size.y, yplanes), range(s.p, s.r, size.z, zplanes)};
		fwrite(r, 8, 3, o);
	}
}
} // namespace pin

namespace Lumix::os { // math.cpp's rand() seeds from the timer (unused here)
u64 Timer::getRawTimestamp() { return 1; }
}

template <typename T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
	v.resize(n ? n : 1);
	return !n || fread(v.data(), sizeof(T), n, f) == n;
}

// in: u32 w, h; DVec3 cam; ShiftedFrustum; u32 n + n x Transform; u32 n + n x {color[3], intensity, range, fov, attenuation_param, flags};
//     u32 n + n x i32 listed; u32 n + n x EnvironmentProbe + n x i32; u32 n + n x {half_extents[3], texture_id, flags} + n x i32;
//     u32 n + n x {pos[3], r}
// out: see the end of pin::run
int main(int argc, char** argv) {
	using namespace Lumix;
	FILE* f = fopen(argv[1], "rb");
	FILE* o = fopen(argv[2], "wb");
	if (!f || !o) return 1;
	u32 wh[2], n;
	pin::CameraParams cp;
	if (fread(wh, 4, 2, f) != 2 || fread(&cp.pos, 8, 3, f) != 3 || fread(&cp.frustum, 256, 1, f) != 1) return 1;
	std::vector<Transform> tr;
	if (fread(&n, 4, 1, f) != 1 || !rd(f, tr, n)) return 1;
	struct PL { float color[3], intensity, range, fov, attenuation_param; u32 flags; };
	std::vector<PL> pl_in;
	if (fread(&n, 4, 1, f) != 1 || !rd(f, pl_in, n)) return 1;
	std::vector<PointLight> pl(pl_in.size());
	for (size_t i = 0; i < n; ++i) {
		pl[i].color = Vec3(pl_in[i].color[0], pl_in[i].color[1], pl_in[i].color[2]);
		pl[i].intensity = pl_in[i].intensity;
		pl[i].range = pl_in[i].range;
		pl[i].fov = pl_in[i].fov;
		pl[i].attenuation_param = pl_in[i].attenuation_param;
		pl[i].flags = (PointLight::Flags)pl_in[i].flags;
	}
	std::vector<EntityRef> listed, env_e, refl_e;
	u32 n_listed, n_env, n_refl, n_spheres;
	if (fread(&n_listed, 4, 1, f) != 1 || !rd(f, listed, n_listed)) return 1;
	std::vector<EnvironmentProbe> env;
	if (fread(&n_env, 4, 1, f) != 1 || !rd(f, env, n_env) || !rd(f, env_e, n_env)) return 1;
	struct RP { float half_extents[3]; u32 texture_id, flags; };
	std::vector<RP> refl_in;
	if (fread(&n_refl, 4, 1, f) != 1 || !rd(f, refl_in, n_refl) || !rd(f, refl_e, n_refl)) return 1;
	std::vector<ReflectionProbe> refl(refl_in.size());
	for (size_t i = 0; i < n_refl; ++i) {
		refl[i].half_extents = Vec3(refl_in[i].half_extents[0], refl_in[i].half_extents[1], refl_in[i].half_extents[2]);
		refl[i].texture_id = refl_in[i].texture_id;
		refl[i].flags = (ReflectionProbe::Flags)refl_in[i].flags;
	}
	std::vector<pin::Sphere> spheres;
	if (fread(&n_spheres, 4, 1, f) != 1 || !rd(f, spheres, n_spheres)) return 1;
	pin::World world{tr.data()};
	pin::Module module{pl.data(), Span<const ReflectionProbe>(refl.data(), (u64)n_refl), Span<const EnvironmentProbe>(env.data(), (u64)n_env),
	                   Span<EntityRef>(refl_e.data(), (u64)n_refl), Span<EntityRef>(env_e.data(), (u64)n_env)};
	spheres.resize(n_spheres);
	listed.resize(n_listed);
	pin::FrameAllocator frame_allocator;
	const pin::ViewportSize viewport{(int)wh[0], (int)wh[1]};
	std::vector<pin::ClusterLight> lights(n_listed ? n_listed : 1);
	memset((void*)lights.data(), 0, lights.size() * sizeof(pin::ClusterLight));
	pin::run(&module, world, frame_allocator, cp, viewport, listed, (i32)n_listed, lights.data(), spheres, o);
	fclose(o);
	return 0;
}
"""


def _block(text, anchor):
    """the brace-matched body (without its braces) of the block that `anchor` opens"""
    a = text.index(anchor)
    i = text.index("{", a + len(anchor) - 1)
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
    raise AssertionError("unbalanced block after " + anchor)


def _between(body, first, behind, last=None):
    """body[first anchor : `behind` anchor) - or through the end of the `last` anchor; each anchor must occur exactly once"""
    for anchor in (first, behind or last):
        assert body.count(anchor) == 1, "the anchor moved: " + anchor
    a = body.index(first)
    b = body.index(behind) if behind else body.index(last) + len(last)
    assert a < b
    return body[a:b]


def slice_reference(out):
    pc = open(os.path.join(REF, "src", "renderer", "pipeline.cpp")).read()
    body = _block(pc, "void fillClusters(DrawStream& stream, const CameraParams& cp) {")
    structs = _between(body, "struct ClusterLight {", "ArenaAllocator& frame_allocator")
    for name in ("struct ClusterLight {", "struct Cluster {", "struct ClusterEnvProbe {", "struct ClusterReflProbe {"):
        assert structs.count(name) == 1, name
    size = _between(body, "const IVec3 size(", "const u32 clusters_count =")
    assert size.count("m_viewport.w + 63") == 1 and size.count("m_viewport.h + 63") == 1 and size.rstrip().endswith("16);")
    clusters = _between(body, "const u32 clusters_count =", "const DVec3 cam_pos = cp.pos;")
    assert clusters.count(";") == 3 and "frame_allocator.allocate(" in clusters and "memset(clusters, 0," in clusters
    cam = _between(body, "const DVec3 cam_pos = cp.pos;", None, "const DVec3 cam_pos = cp.pos;")
    each = _block(body, "light_entities->forEach([&](EntityRef e){")
    light = _between(each, "PointLight& pl = m_module->getPointLight(e);", None, "light.attenuation_param = pl.attenuation_param;")
    for stmt in ("ClusterLight& light = lights[i];", "light.radius = pl.range;", "const DVec3 light_pos = world.getPosition(e);", "light.pos = Vec3(light_pos - cam_pos);",
                 "light.rot = world.getRotation(e);", "light.fov = pl.fov;", "light.color = pl.color * pl.intensity;"):
        assert stmt in light, stmt
    assert "atlas" not in light
    planes = _between(body, "const Span<const ReflectionProbe> module_refl_probes", "ASSERT(lengthOf(xplanes)")
    assert planes.count("frame_allocator.allocate(") == 2 and "const ShiftedFrustum& frustum = cp.frustum;" in planes and "Vec4 xplanes[65];" in planes
    assert planes.count("makePlane(") == 3 and planes.count("for (") == 3 and "powf(" in planes and planes.rstrip().endswith("}")
    probes = _between(body, "const Span<EntityRef> refl_probe_entities", "auto range = [](")
    assert probes.count("sort(") == 2 and probes.count("conjugated()") == 2 and probes.count("ENABLED)) continue;") == 2
    rng = _between(body, "auto range = [](", "// TODO tighter fit")
    assert rng.count("planeDist(") == 3 and rng.rstrip().endswith("};")
    binning = _between(body, "auto for_each_light_pair", "bind(m_cluster_buffers.lights")
    assert binning.count("for_each_light_pair(") == 2 and binning.count("for_each_env_probe_pair(") == 2 and binning.count("for_each_refl_probe_pair(") == 2
    assert "frame_allocator.allocate(offset * sizeof(i32)" in binning and "cluster.offset -= " in binning
    for name, text in (("cl_structs.inc", structs), ("cl_size.inc", size), ("cl_clusters.inc", clusters), ("cl_cam.inc", cam), ("cl_light.inc", light), ("cl_planes.inc", planes), ("cl_probes.inc", probes), ("cl_range.inc", rng),
                       ("cl_binning.inc", binning)):
        open(os.path.join(out, name), "w").write(text + "\n")


def have_reference():
    return os.path.isfile(os.path.join(REF, "src", "renderer", "pipeline.cpp"))


def build_harness(d):
    """Slices the reference into `d` and compiles the harness there -> the program's path."""
    d = str(d)
    core = os.path.join(d, "core")
    shutil.copytree(os.path.join(REF, "src", "core"), core)  # core/sync.h:20-24 is `#error "Not implemented"` on Linux (oracle/Makefile)
    sync = os.path.join(core, "sync.h")
    open(sync, "w").write(open(os.path.join(REF, "src", "core", "sync.h")).read().replace('#error "Not implemented"', "pthread_rwlock_t lock;", 1))
    gen = os.path.join(d, "gen")
    os.mkdir(gen)
    slice_reference(gen)
    open(os.path.join(d, "harness.cpp"), "w").write(HARNESS)
    inc = ["-I" + d, "-I" + gen, "-I" + os.path.join(REF, "src"), "-I" + os.path.join(REF, "external")]
    objs = []
    for path in (os.path.join(d, "harness.cpp"), os.path.join(REF, "src", "core", "math.cpp"), os.path.join(REF, "src", "core", "geometry.cpp")):
        obj = os.path.join(d, os.path.basename(path) + ".o")
        r = subprocess.run(["g++"] + FLAGS + inc + ["-c", path, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = os.path.join(d, "cluster_ref")
    r = subprocess.run(["g++"] + objs + ["-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def ref_harness(tmp_path_factory):
    if not have_reference():
        pytest.skip("no reference tree on this machine")
    d = tmp_path_factory.mktemp("cluster_ref")
    return build_harness(d), str(d)


def _counted(a, dtype):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    return np.uint32(len(a)).tobytes() + a.tobytes()


def run_ref(ref_harness, view, entities=(), transforms=None, light_table=None, env=None, env_entities=None, refl=None, refl_entities=None, spheres=None):
    """The reference's statements on one view -> dict(size, xplanes, yplanes, zplanes, lights, env_probes, refl_probes, clusters, map,
    ranges[n_spheres, 3, 2]). Every listed entity and every probe's entity must lie inside the tables."""
    exe, d = ref_harness
    v = np.ascontiguousarray(view, api.CLUSTER_VIEW).reshape(-1)[0]
    transforms = np.zeros(0, api.TRANSFORM) if transforms is None else np.ascontiguousarray(transforms, api.TRANSFORM)
    light_table = np.zeros(0, api.POINT_LIGHT) if light_table is None else light_table
    entities = np.ascontiguousarray(entities, np.int32)
    env = np.zeros(0, api.ENV_PROBE) if env is None else np.ascontiguousarray(env, api.ENV_PROBE)
    refl = np.zeros(0, api.REFL_PROBE) if refl is None else np.ascontiguousarray(refl, api.REFL_PROBE)
    env_entities = np.ascontiguousarray([] if env_entities is None else env_entities, np.int32)
    refl_entities = np.ascontiguousarray([] if refl_entities is None else refl_entities, np.int32)
    spheres = np.zeros((0, 4), np.float32) if spheres is None else np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    assert len(env) == len(env_entities) and len(refl) == len(refl_entities)
    assert len(light_table) == len(transforms) or not len(entities)
    for e in (entities, env_entities, refl_entities):
        assert not len(e) or (e.min() >= 0 and e.max() < len(transforms)), "the reference has no entity outside its world"
    job = np.array([v["viewport_w"], v["viewport_h"]], np.uint32).tobytes() + np.asarray(v["camera_pos"], np.float64).tobytes() + v["frustum"].tobytes()
    job += _counted(transforms, api.TRANSFORM) + _counted(light_table, api.POINT_LIGHT) + _counted(entities, np.int32)
    job += np.uint32(len(env)).tobytes() + env.tobytes() + env_entities.tobytes()
    refl_in = np.zeros(len(refl), np.dtype([("half_extents", "<f4", 3), ("texture_id", "<u4"), ("flags", "<u4")]))
    for k in refl_in.dtype.names:
        refl_in[k] = refl[k]
    job += np.uint32(len(refl)).tobytes() + refl_in.tobytes() + refl_entities.tobytes()
    job += np.uint32(len(spheres)).tobytes() + spheres.tobytes()
    open(os.path.join(d, "job.bin"), "wb").write(job)
    subprocess.run([exe, os.path.join(d, "job.bin"), os.path.join(d, "out.bin")], check=True, timeout=300)
    b = open(os.path.join(d, "out.bin"), "rb").read()
    at = 0

    def take(dtype, n, shape=None):
        nonlocal at
        a = np.frombuffer(b, dtype, n, at).copy()
        at += a.nbytes
        return a if shape is None else a.reshape(shape)

    size = tuple(int(x) for x in take(np.int32, 3))
    out = {"size": size}
    out["xplanes"], out["yplanes"], out["zplanes"] = (take(np.float32, 4 * (s + 1), (s + 1, 4)) for s in size)
    out["lights"] = take(api.CLUSTER_LIGHT, len(entities))
    out["env_probes"] = take(api.CLUSTER_ENV_PROBE, len(env))
    out["refl_probes"] = take(api.CLUSTER_REFL_PROBE, len(refl))
    out["clusters"] = take(api.CLUSTER, size[0] * size[1] * size[2])
    out["map"] = take(np.int32, int(take(np.uint32, 1)[0]))
    out["ranges"] = take(np.int32, 6 * len(spheres), (len(spheres), 3, 2))
    assert at == len(b)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


# ---- planes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["perspective", "ortho"])
@pytest.mark.parametrize("w,h", [(1920, 1080), (128, 64), (65, 1), (4096, 4096)])
def test_planes_of_the_oracle_and_of_the_library_equal_the_reference(ref_harness, w, h, kind):
    from tests import test_cluster_planes as P

    assert (w, h) in P.VIEWPORTS
    if not os.path.exists(api.LIB_PATH):
        from lumixengine_amd import build

        build.build()
    f = P.frusta(api, w, h)[kind]
    ref = run_ref(ref_harness, api.cluster_view(P.CAM, f, w, h))
    size, xp, yp, zp = CO.planes(f, w, h)
    got = api.clusters_planes(f, w, h)[0]
    assert ref["size"] == size == tuple(int(x) for x in got["size"])
    for name, oracle in (("xplanes", xp), ("yplanes", yp), ("zplanes", zp)):
        want = ref[name]
        assert np.isfinite(want).all() and np.abs(want[:, :3]).max() > 0.1, name
        assert bits(oracle) == bits(want), f"{name}: the oracle against the reference"
        assert bits(got[name][: len(want)]) == bits(want), f"{name}: lmx_clusters_planes against the reference"


# ---- range() ---------------------------------------------------------------------------------------------------------------------
def seeded_spheres(view, w, h, seed, n=3000):
    """[n, 4] spheres (pos relative to the camera, r) for range() on the view's planes: in and around the frustum with radii from tiny to
    scene-wide; spheres whose distance to some plane of each axis EQUALS +r and -r (built as cluster_oracle.hand_made builds
    them: plane_dists, then the radius set to that distance) and their nextafter neighbours; NaN, infinities, negative and zero radii."""
    rng = np.random.default_rng(seed)
    size, xp, yp, zp = CO.planes(view["frustum"][0], w, h)
    depth = np.exp(rng.uniform(np.log(0.05), np.log(30000.0), n))
    pos = np.stack([rng.uniform(-1.2, 1.2, n) * depth, rng.uniform(-1.2, 1.2, n) * depth, -depth], axis=1).astype(np.float32)
    behind = rng.random(n) < 0.05
    pos[behind, 2] = rng.uniform(0, 50, behind.sum())
    r = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)).astype(np.float32)
    r[rng.random(n) < 0.02] = 1.0e5
    exact = {}
    k = 0
    for axis, pl in enumerate((xp, yp, zp)):
        d = CO.plane_dists(pl, pos[n // 2 :])
        for j in rng.choice(len(pl), min(len(pl), 12), replace=False):
            for sign in (1, -1):  # a sphere on either side of plane j: dist == +r and dist == -r
                src = np.flatnonzero(np.isfinite(d[:, j]) & (np.sign(d[:, j]) == sign))
                if not len(src):
                    continue
                dist = abs(d[src[0], j])
                for variant, rad in enumerate((dist, np.nextafter(dist, np.float32(0)), np.nextafter(dist, np.float32(np.inf)))):  # and a step to either side
                    pos[k], r[k] = pos[n // 2 + src[0]], rad
                    if variant == 0:
                        exact[k] = (axis, int(j), float(d[src[0], j]))
                    k += 1
    special = [((np.nan, 0, -1), 1), ((0, np.nan, -1), 1), ((0, 0, np.nan), 1), ((0, 0, -1), np.nan), ((np.inf, 0, -1), 1), ((0, -np.inf, -1), 1), ((0, 0, -np.inf), 1),
               ((0, 0, np.inf), 1), ((0, 0, -1), np.inf), ((0, 0, -1), -np.inf), ((np.inf, 0, -1), np.inf), ((0, 0, -5), -1.0), ((0, 0, -5), -0.0), ((0, 0, -5), 0.0),
               ((1e3, 0, -5), -1e4), ((0, 0, 5), -10.0), ((0, 0, -5), -1e-3)]
    for i, (p, rad) in enumerate(special):
        pos[n - 1 - i], r[n - 1 - i] = p, rad
    assert k < n // 2
    return np.concatenate([pos, r[:, None]], axis=1).astype(np.float32), exact


def test_range_of_the_hand_made_spheres_equals_the_reference(ref_harness):
    view, names, tr, lights, radius = CO.hand_made()
    rec = CO.light_records(np.arange(len(tr), dtype=np.int32), tr, lights, None, CO.CAM_POS)
    spheres = np.concatenate([rec["pos"], rec["radius"][:, None]], axis=1)
    assert len(spheres) == 15 and np.isnan(spheres[names.index("nan"), 0])  # (the sixteenth, past the tables, reads as zeros: it closes the list)
    spheres = np.concatenate([spheres, np.zeros((1, 4), np.float32)])
    ref = run_ref(ref_harness, view, spheres=spheres)
    size, xp, yp, zp = CO.planes(view["frustum"][0], 128, 64)
    assert CO.ranges(size, xp, yp, zp, spheres[:, :3], spheres[:, 3]).tolist() == ref["ranges"].tolist()
    for i, s in enumerate(spheres):  # the scalar statement of the oracle too
        for axis, pl in enumerate((xp, yp, zp)):
            assert list(CO.axis_range(CO.plane_dists(pl, s[None, :3])[0], s[3], size[axis])) == ref["ranges"][i, axis].tolist(), (names[i], axis)
    by = dict(zip(names, ref["ranges"].tolist()))
    assert by["dist_eq_r"][2][0] == 2 and by["dist_gt_r"][2][0] == 3 and by["dist_eq_minus_r"][2][1] == 5 and by["dist_lt_minus_r"][2][1] == 4
    assert by["nan"] == [[0, 2], [0, 1], [0, 16]]


@pytest.mark.parametrize("w,h", [(128, 64), (4096, 4096)])
def test_range_of_seeded_spheres_equals_the_reference(ref_harness, w, h):
    view = CO.view(w, h)
    spheres, exact = seeded_spheres(view, w, h, seed=w)
    size, xp, yp, zp = CO.planes(view["frustum"][0], w, h)
    assert size == ((2, 1, 16) if w == 128 else (64, 64, 16))
    # what the set is about: distances that equal +r and -r on every axis, and the special values
    for axis, pl in enumerate((xp, yp, zp)):
        signs = {np.sign(d) for k, (a, j, d) in exact.items() if a == axis and CO.plane_dists(pl, spheres[k : k + 1, :3])[0][j] == np.float32(d) and abs(np.float32(d)) == spheres[k, 3]}
        assert signs == {1.0, -1.0}, (axis, signs)
    assert np.isnan(spheres).any() and np.isinf(spheres).any() and (spheres[:, 3] < 0).any() and (spheres[:, 3] == 0).any()
    ref = run_ref(ref_harness, view, spheres=spheres)
    got = CO.ranges(size, xp, yp, zp, spheres[:, :3], spheres[:, 3])
    bad = np.flatnonzero((got != ref["ranges"]).any(axis=(1, 2)))
    assert not len(bad), (len(bad), spheres[bad[0]].tolist(), got[bad[0]].tolist(), ref["ranges"][bad[0]].tolist())
    assert (got[:, :, 0] == -1).any() and (got[:, 0, 1] == size[0]).any() and len({tuple(r) for r in got[:, 2].tolist()}) > 30
    for i in np.random.default_rng(1).choice(len(spheres), 40, replace=False):  # the scalar statement agrees with the vectorised one
        for axis, pl in enumerate((xp, yp, zp)):
            assert list(CO.axis_range(CO.plane_dists(pl, spheres[i : i + 1, :3])[0], spheres[i, 3], size[axis])) == got[i, axis].tolist()


# ---- the whole pass --------------------------------------------------------------------------------------------------------------
RECORD_FIELDS = {"lights": ("pos", "radius", "rot", "color", "attenuation_param", "fov"),  # (atlas_idx: deviation 3; the padding: no slice writes it)
                 "env_probes": ("pos", "rot", "inner_range", "outer_range", "sh_coefs"), "refl_probes": ("pos", "layer", "rot", "half_extents")}


def assert_same_pass(ref, want, what):
    assert ref["size"] == want["size"], what
    for name, fields in RECORD_FIELDS.items():
        assert len(ref[name]) == len(want[name]), (what, name)
        for k in fields:
            assert np.ascontiguousarray(ref[name][k]).tobytes() == np.ascontiguousarray(want[name][k]).tobytes(), f"{what}: {name}.{k}"
    assert ref["clusters"].tobytes() == want["clusters"].tobytes(), what + ": clusters"
    assert ref["map"].tobytes() == want["map"].tobytes(), what + ": map"


@functools.lru_cache(maxsize=None)
def pinned_probes(n_env=9, n_refl=7):
    """every probe enabled, volume products pairwise distinct, the second of each kind scene-wide"""
    p = CO.probe_tables(n_env, n_refl, seed=21, wide=(1,))
    for kind, field in (("env", "outer_range"), ("refl", "half_extents")):
        assert (p[kind]["flags"] & api.PROBE_ENABLED).all()
        assert len(set((p[kind][field][:, 0] * p[kind][field][:, 1] * p[kind][field][:, 2]).tolist())) == len(p[kind])
    return p


def whole_pass_case(name):
    sc = CO.scene()
    if name == "seeded 1920x1080":
        view, listed, _, _ = CO.seeded_case()  # (its own probes hold disabled ones and ties: the pinned set stands in)
        assert len(listed) == 3000
    elif name == "128x64":
        view, listed = CO.view(128, 64), np.random.default_rng(31).choice(CO.N_ENTITIES, 600, replace=False).astype(np.int32)
    else:
        view, listed = CO.view(4096, 4096), np.random.default_rng(32).choice(CO.N_ENTITIES, 300, replace=False).astype(np.int32)
    return sc, view, listed, pinned_probes()


@pytest.mark.parametrize("name", ["seeded 1920x1080", "128x64", "4096x4096"])
def test_whole_pass_equals_the_reference(ref_harness, name):
    sc, view, listed, probes = whole_pass_case(name)
    ref = run_ref(ref_harness, view, listed, sc["transforms"], sc["lights"], **probes)
    want = CO.fill_clusters(view, listed, sc["transforms"], sc["lights"], None, **probes)
    assert_same_pass(ref, want, name)
    cl = want["clusters"]
    assert len(want["map"]) > 1000 and cl["lights_count"].max() > 1 and cl["env_probes_count"].max() > 1 and cl["refl_probes_count"].max() > 1
    assert cl["env_probes_count"].min() >= 1 and cl["refl_probes_count"].min() >= 1  # the scene-wide probes are everywhere
    if name == "4096x4096":
        assert want["size"] == (64, 64, 16) and (want["ranges"][:, 0] == (0, 64)).all(axis=1).any()


def test_records_equal_the_reference_at_the_fp64_camera(ref_harness):
    """Vec3(pos - cam_pos) is one rounding of an fp64 difference at CAM_POS = (1e6, 50, -1e6); the probes come out in ascending volume."""
    sc = CO.scene()
    view = CO.view(128, 64)
    assert tuple(view["camera_pos"][0]) == CO.CAM_POS
    probes = pinned_probes(12, 12)
    listed = np.arange(CO.N_ENTITIES, dtype=np.int32)
    ref = run_ref(ref_harness, view, listed, sc["transforms"], sc["lights"], **probes)
    want = CO.fill_clusters(view, listed, sc["transforms"], sc["lights"], None, **probes)
    assert_same_pass(ref, want, "records")
    i = 7
    assert want["lights"]["pos"][i].tolist() != (sc["transforms"]["pos"][i].astype(np.float32) - np.asarray(CO.CAM_POS, np.float32)).tolist()
    for name, field in (("env_probes", "outer_range"), ("refl_probes", "half_extents")):
        e = ref[name][field]
        assert len(e) == 12 and (np.diff(e[:, 0] * e[:, 1] * e[:, 2]) > 0).all()
    assert probes["env"]["outer_range"].tolist() != ref["env_probes"]["outer_range"].tolist()  # (the module order is not the output order)
