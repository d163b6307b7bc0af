"""The mirrors tests/test_gpu_grass.py places its edges with - api.GRASS_WINDOW, the cull's block, the slot size - and the records of the
grass entry points are held to lmx_grass.h and the public headers."""
import os
import re
import subprocess

from lumixengine_amd import api
from tests.test_ray_im_constants import CSRC, ROOT, literal


def test_launch_constants_mirror_the_header():
    g_h = open(os.path.join(CSRC, "lmx_grass.h")).read()
    for name in ("GRASS_WINDOW", "GRASS_CULL_BLOCK"):
        assert literal(g_h, name) == getattr(api, name), name
    assert api.GRASS_CULL_BLOCK % 64 == 0


def test_enums_mirror_the_public_header():
    t_h = open(os.path.join(ROOT, "include", "lmx_types.h")).read()
    for name in ("GRASS_ROTATION_Y_UP", "GRASS_ROTATION_ALL_RANDOM"):
        found = re.findall(r"^#define\s+LMX_" + name + r"\s+(\d+)u\b", t_h, re.M)
        assert len(found) == 1 and int(found[0]) == getattr(api, name), name
    for name in ("GRASS_MAX_TERRAINS", "GRASS_MAX_TYPES", "GRASS_SAMPLES", "GRASS_SLOT_INSTANCES"):
        found = re.findall(r"\bLMX_" + name + r"\s*=\s*(\d+)", t_h)
        assert len(found) == 1 and int(found[0]) == getattr(api, name), name
    assert api.GRASS_SLOT_INSTANCES == 2 * api.GRASS_SAMPLES


def test_records_match_the_c_header(tmp_path):
    structs = {"LmxGrassType": (api.GRASS_TYPE, ["spacing", "distance", "rotation_mode", "usable"]),
               "LmxGrassTerrain": (api.GRASS_TERRAIN, ["heightmap", "splat_width", "splat_height", "splat_format", "splat_ready", "splat_texels", "types", "n_types"]),
               "LmxGrassInstance": (api.GRASS_INSTANCE, ["position", "scale", "rotation"]),
               "LmxGrassQuad": (api.GRASS_QUAD, ["aabb_min", "aabb_max", "ij", "type", "instances_count", "terrain", "slot"]),
               "LmxGrassView": (api.GRASS_VIEW, ["frustum", "viewport_pos", "lod_multiplier"]),
               "LmxGrassDraw": (api.GRASS_DRAW, ["quad", "slot", "terrain", "type", "instance_count", "distance"]),
               "LmxGrassCounts": (api.GRASS_COUNTS, ["draws", "culled", "instances", "live"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lumix_mi355.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        lines += [f'printf(" %zu", offsetof({name}, {f}));' for f in fields]
        lines.append('printf("\\n");')
    lines.append('printf("LmxGrassDevice %zu %zu %zu\\n", sizeof(LmxGrassDevice), offsetof(LmxGrassDevice, d_counts), offsetof(LmxGrassDevice, n_live));')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()}
    for name, (dtype, fields) in structs.items():
        assert got[name] == [dtype.itemsize] + [dtype.fields[f][1] for f in fields], name
    import ctypes as C

    assert got["LmxGrassDevice"] == [C.sizeof(api.LmxGrassDevice), api.LmxGrassDevice.d_counts.offset, api.LmxGrassDevice.n_live.offset]
    assert (api.GRASS_TERRAIN.itemsize, api.GRASS_INSTANCE.itemsize, api.GRASS_QUAD.itemsize, api.GRASS_VIEW.itemsize, api.GRASS_DRAW.itemsize) == (80, 32, 48, 288, 24)
