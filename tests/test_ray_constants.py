"""api.RAY_* mirror the launch geometry of ray_kernels.hip (lmx_kernels.h). tests/test_gpu_rays.py computes the work-item, wave, block and
tile edges of both phases from the mirrors: retuned kernels either move that test along or fail here. The guard, the flags and the record
sizes are held to their headers the same way."""
import os
import re

from lumixengine_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ray_launch_geometry_mirrors_the_header():
    text = open(os.path.join(ROOT, "lumixengine_amd", "csrc", "lmx_kernels.h")).read()
    for name in ("RAY_BLOCK", "RAY_BROAD_RAYS", "RAY_BROAD_GRID", "RAY_RUN", "RAY_NARROW_SPLIT", "RAY_NARROW_GRID", "RAY_MAX_BONES"):
        found = re.findall(r"^constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)u?\s*;", text, re.M)
        assert len(found) == 1, f"{name}: expected one `constexpr uint32_t {name} = <literal>;` in lmx_kernels.h, found {len(found)}"
        assert int(found[0]) == getattr(api, name), f"api.{name} = {getattr(api, name)}, lmx_kernels.h says {found[0]}"
    assert api.RAY_NARROW_GRID % api.RAY_NARROW_SPLIT == 0 and api.RAY_BLOCK % 64 == 0 and api.RAY_BROAD_RAYS <= api.RAY_BLOCK


def test_ray_guard_flags_and_records_mirror_the_headers():
    ctx_h = open(os.path.join(ROOT, "lumixengine_amd", "csrc", "lmx_context.h")).read()
    assert [int(x) for x in re.findall(r"constexpr\s+size_t\s+RAYS_GUARD_BYTES\s*=\s*(\d+)\s*;", ctx_h)] == [api.RAYS_GUARD_BYTES]
    assert api.RAYS_GUARD_BYTES % api.RAY_CANDIDATE.itemsize == 0
    pub = open(os.path.join(ROOT, "include", "lumix_mi355.h")).read()
    assert [int(x) for x in re.findall(r"LMX_RAY_INSTANCE_ENABLED\s*=\s*1\s*<<\s*(\d+)", pub)] == [api.RAY_INSTANCE_ENABLED.bit_length() - 1]
    assert [int(x) for x in re.findall(r"LMX_RAY_INSTANCE_VALID\s*=\s*1\s*<<\s*(\d+)", pub)] == [api.RAY_INSTANCE_VALID.bit_length() - 1]
    assert (api.RAY.itemsize, api.RAY_HIT.itemsize, api.RAY_MODEL.itemsize, api.RAY_CANDIDATE.itemsize, api.RAYS_COUNTS.itemsize) == (48, 24, 44, 48, 12)


def test_ray_records_match_the_c_header(tmp_path):
    import subprocess

    structs = {"LmxRay": (api.RAY, ["origin", "dir", "t_max", "ignore"]), "LmxRayHit": (api.RAY_HIT, ["is_hit", "entity", "mesh", "triangle", "t", "t_model"]),
               "LmxRayModel": (api.RAY_MODEL, ["aabb_min", "aabb_max", "origin_radius", "ready", "first_mesh", "mesh_count", "lod0_from"]),
               "LmxRaysCounts": (api.RAYS_COUNTS, ["rays", "candidates", "overflow"])}
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
