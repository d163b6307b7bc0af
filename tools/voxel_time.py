#!/usr/bin/env python
"""Times Voxels on the device (lmx_voxels_*) on a sphere of 2 000 triangles:
  the importer's shape  max_res 64 (a grid of 67^3), 32 rays: ModelImporter::bakeVertexAO's voxelize, computeAO(32), blurAO and the bake of the
                        mesh's vertices, with k_voxel_ao's bit mask staged in LDS and with LMX_VOXELS_OPT_AO_LDS = 0 (bytes in global memory);
  a 128 grid            max_res 128 (131^3 cells): over what the LDS form stages, so the global-memory form alone.
--rounds rounds of --steps runs each; per step the wall time of each call up to the synchronise behind it. One JSON line with the medians, and
profiles/voxels/README.md (--out) with the same numbers as a table next to the reference's one-thread time, where --reference-ms gives it
(tests/test_voxel_oracle_vs_ref.py prints that figure where the reference tree exists). No bar is fixed.

    python tools/voxel_time.py [--steps 5] [--rounds 3] [--out profiles/voxels/README.md] [--reference-ms 3597]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumixengine_amd import api  # noqa: E402
from tests import voxel_oracle as VO  # noqa: E402  (the sphere mesh of the tests)

RAYS = 32
SEED = (0xC0FFEE, 0xBADF00D)


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shape(ctx, mesh, max_res, lds, steps, rounds):
    v = api.Voxels(ctx)
    v.setOption(api.VOXELS_OPT_AO_LDS, 1 if lds else 0)
    per = {"voxelize": [], "compute_ao": [], "blur_ao": [], "bake": []}
    for r in range(rounds + 1):  # (round 0 warms up)
        one = {k: [] for k in per}
        for _ in range(steps):
            one["voxelize"].append(timed(ctx, lambda: v.voxelize([mesh], max_res)))
            one["compute_ao"].append(timed(ctx, lambda: v.computeAO(RAYS, *SEED)))
            one["blur_ao"].append(timed(ctx, lambda: v.blurAO()))
            one["bake"].append(timed(ctx, lambda: v.bakeVertexAO(mesh[0], 0.0)))
        if r:
            for k in per:
                per[k].append(float(np.median(one[k])))
    res = v.info()["resolution"].tolist()
    occupied = int(v.read().sum())
    v.close()
    out = {"max_res": max_res, "resolution": res, "cells": int(np.prod(res)), "occupied": occupied, "rays": RAYS, "ao_form": "lds" if lds else "global"}
    for k, ms in per.items():
        out[k + "_ms"] = float(np.median(ms))
        out[k + "_round_medians_ms"] = ms
    return out


def readme(rows, args):
    lines = ["# Voxels on the device: timings", "",
             "Written by `tools/voxel_time.py` (DESIGN.md §4.21). A sphere of 2 000 triangles; medians over %d rounds of %d runs, wall time of each call" % (args.rounds, args.steps),
             "up to the synchronise behind it (host-side validation, uploads and the launch included). `lds` / `global`: the form of `k_voxel_ao`.", "",
             "| max_res | grid | AO form | voxelize ms | computeAO(32) ms | blurAO ms | bake ms |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %s | %s | %.3f | %.3f | %.3f | %.3f |" % (r["max_res"], " x ".join(str(x) for x in r["resolution"]), r["ao_form"], r["voxelize_ms"], r["compute_ao_ms"],
                                                                 r["blur_ao_ms"], r["bake_ms"]))
    lines.append("")
    if args.reference_ms is not None:
        lines.append("The reference's `computeAO(32)` on the 67^3 grid of the same mesh, one thread of the development machine's CPU: %.0f ms" % args.reference_ms)
        lines.append("(tests/test_voxel_oracle_vs_ref.py prints it). It is the CPU side of the comparison, not a bar.")
    else:
        lines.append("The reference's one-thread time: not measured in this run.")
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxels", "README.md"))
    ap.add_argument("--reference-ms", type=float, default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    mesh = VO.sphere_mesh(26, 40)
    rows = [shape(ctx, mesh, 64, True, a.steps, a.rounds), shape(ctx, mesh, 64, False, a.steps, a.rounds), shape(ctx, mesh, 128, False, a.steps, a.rounds)]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(readme(rows, a))
    print(json.dumps({"tool": "voxel_time", "steps": a.steps, "rounds": a.rounds, "shapes": rows}))
