"""The mirrors tests/test_gpu_rays_scene.py places its edges with - api.RAY_TERRAIN_CHUNK, the grids, the overflow bit - and the records of
the procedural-geometry, terrain and merge stages are held to lmx_kernels.h and the public headers."""
import os
import re
import subprocess

from lumixengine_amd import api
from tests.test_ray_im_constants import CSRC, ROOT, literal


def test_launch_constants_mirror_the_header():
    k_h = open(os.path.join(CSRC, "lmx_kernels.h")).read()
    for name in ("RAY_PG_BROAD_GRID", "RAY_TERRAIN_CHUNK", "RAY_TERRAIN_GRID", "RAY_MAX_TERRAINS"):
        assert literal(k_h, name) == getattr(api, name), name
    assert re.search(r"RAYS_PG_OVERFLOW\s*=\s*4\b", k_h) and api.RAYS_PG_OVERFLOW == 4
    # one step of a chunk per lane of the wave that walks a (ray, terrain) pair; whole waves per block
    assert api.RAY_TERRAIN_CHUNK == 64 and api.RAY_BLOCK % api.RAY_TERRAIN_CHUNK == 0
    src = open(os.path.join(CSRC, "ray_scene_kernels.hip")).read()
    assert "static_assert(RAY_TERRAIN_CHUNK == WAVE" in src


def test_enums_mirror_the_public_header():
    t_h = open(os.path.join(ROOT, "include", "lmx_types.h")).read()
    for name in ("RAY_TERRAIN_R16", "RAY_TERRAIN_RGBA8", "RAY_HIT_MODEL_INSTANCE", "RAY_HIT_INSTANCED_MODEL", "RAY_HIT_PROCEDURAL_GEOM", "RAY_HIT_TERRAIN"):
        found = re.findall(r"^#define\s+LMX_" + name + r"\s+(\d+)u\b", t_h, re.M)
        assert len(found) == 1 and int(found[0]) == getattr(api, name), name


def test_records_match_the_c_header(tmp_path):
    structs = {"LmxRayProcGeom": (api.RAY_PROC_GEOM, ["entity", "triangles", "aabb_min", "aabb_max", "vertex_data", "vertex_bytes", "stride", "index_data", "index_bytes", "index_count"]),
               "LmxRayTerrain": (api.RAY_TERRAIN, ["entity", "width", "height", "format", "scale", "ready", "texels"]),
               "LmxRayPgHit": (api.RAY_PG_HIT, ["is_hit", "entity", "geom", "triangle", "t"]),
               "LmxRayTerrainHit": (api.RAY_TERRAIN_HIT, ["is_hit", "entity", "terrain", "hx", "hz", "tri", "t"]),
               "LmxRaySceneHit": (api.RAY_SCENE_HIT, ["is_hit", "component", "entity", "index", "sub", "t"]),
               "LmxRaysSceneCounts": (api.RAYS_SCENE_COUNTS, ["rays", "candidates", "overflow"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lumix_mi355.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        lines += [f'printf(" %zu", offsetof({name}, {f}));' for f in fields]
        lines.append('printf("\\n");')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()}
    for name, (dtype, fields) in structs.items():
        assert got[name] == [dtype.itemsize] + [dtype.fields[f][1] for f in fields], name
    assert (api.RAY_PROC_GEOM.itemsize, api.RAY_TERRAIN.itemsize, api.RAY_PG_HIT.itemsize, api.RAY_TERRAIN_HIT.itemsize, api.RAY_SCENE_HIT.itemsize) == (64, 40, 20, 28, 24)
