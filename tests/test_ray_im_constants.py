"""The mirrors tests/test_gpu_rays_im.py places its edges with - api.IM_TILE, api.RAY_IM_BROAD_GRID, the 256-slot tile of k_imray_broad -
and the records of the instanced-model stage are held to lmx_im.h, lmx_kernels.h and the public headers."""
import os
import re
import subprocess

from lumixengine_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lumixengine_amd", "csrc")


def literal(text, name):
    found = re.findall(r"^constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)u?\s*;", text, re.M)
    assert len(found) == 1, f"{name}: expected one `constexpr uint32_t {name} = <literal>;`, found {len(found)}"
    return int(found[0])


def test_tile_and_grid_mirror_the_headers():
    im_h, k_h = open(os.path.join(CSRC, "lmx_im.h")).read(), open(os.path.join(CSRC, "lmx_kernels.h")).read()
    assert literal(im_h, "IM_TILE") == api.IM_TILE
    assert literal(k_h, "RAY_IM_BROAD_GRID") == api.RAY_IM_BROAD_GRID
    # a 256-slot tile of k_imray_broad is one block of the ray kernels and divides IM_TILE: it never straddles two models
    assert literal(k_h, "RAY_BLOCK") == api.RAY_BLOCK and api.IM_TILE % api.RAY_BLOCK == 0
    src = open(os.path.join(CSRC, "ray_kernels.hip")).read()
    assert "SUB = IM_TILE / RAY_BLOCK" in src and "static_assert(SUB * RAY_BLOCK == IM_TILE" in src
    assert re.search(r"RAYS_IM_OVERFLOW\s*=\s*3\b", k_h) and literal(k_h, "RAY_BLOCK") * 32 == api.IM_TILE


def test_records_match_the_c_header(tmp_path):
    structs = {"LmxRayImHit": (api.RAY_IM_HIT, ["is_hit", "entity", "model", "subindex", "mesh", "triangle", "t", "t_model"]),
               "LmxRaysImCounts": (api.RAYS_IM_COUNTS, ["rays", "candidates", "overflow"])}
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
    assert api.RAY_IM_HIT.itemsize == 32 and api.RAYS_IM_COUNTS.itemsize == 12
