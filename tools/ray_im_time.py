#!/usr/bin/env python
"""Times the instanced-model stage of the batched ray cast: the span of lmx_rays_cast_device's launches with an LmxInstancedModels
attached (k_imray_broad, k_ray_narrow, k_imray_resolve, k_imray_write, then the entity stage over an EMPTY instance table, so the span is
the instanced-model stage plus the entity stage's fixed launches) over --instances instances of four models (a 1 k, a 4 k, a 10 k and a
5 k triangle sphere) scattered through a --box cube around four origins, for batches of 1, 1024 and 65 536 rays from the cube's centre.
Median of --steps, warm (back to back) and behind a 1 GiB scrub of the caches; one JSON line. --plain 1 adds the span of the same cast
with the object detached (the entity stage's fixed cost alone).

    python tools/ray_im_time.py --steps 20 [--instances 1000000] [--rays 1,1024,65536]

The rays are in device memory before the span starts; no count reaches the host inside it. The broad phase is arithmetic, not traffic:
per (ray, instance) pair roughly 30 fp32 operations (rel_pos, the sphere test), 32 B of the instance per RAY_BROAD_RAYS rays and 60 B of
the ray and its base per RAY_BLOCK instances; the two quaternion rotations only for the pairs that pass. The tool reports pairs per ns
next to the span; no bar is fixed. Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run (tools/gpu_cases/rays_im.sh).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ray_time import sphere  # noqa: E402

FP32_OPS_PER_PAIR = 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--instances", type=int, default=1_000_000)
    ap.add_argument("--rays", default="1,1024,65536")
    ap.add_argument("--box", type=float, default=1000.0)
    ap.add_argument("--plain", type=int, default=1)
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api

    n = args.instances
    rng = np.random.default_rng(7)
    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB (torch opens the device before the library does)
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    centre = np.array([1.0e6, 50.0, -1.0e6])
    api.DrawCommands(ctx).setTransforms(np.zeros(1, api.TRANSFORM))
    api.PoseProcessor(ctx).setInstances(np.full(1, -1, np.int32))
    rc = api.RayCaster(ctx)
    shapes = [sphere(23, 23), sphere(46, 45), sphere(72, 70), sphere(51, 50)]
    models = np.zeros(len(shapes), api.RAY_MODEL)
    tris = []
    for k, (pos, idx) in enumerate(shapes):
        models[k]["first_mesh"], models[k]["mesh_count"], models[k]["ready"] = rc.addMesh(pos, idx), 1, 1
        models[k]["aabb_min"], models[k]["aabb_max"], models[k]["origin_radius"] = -1.001, 1.001, 1.001
        tris.append(len(idx) // 3)
    rc.setModels(models)
    rc.setInstances(np.full(1, -1, np.int32), np.zeros(1, np.uint8))  # no model instance: the entity stage runs its launches over nothing
    im = api.InstancedModels(ctx)
    origins = centre + rng.uniform(-5, 5, (len(shapes), 3))
    per_model = [n // len(shapes)] * (len(shapes) - 1) + [n - (len(shapes) - 1) * (n // len(shapes))]
    for k, count in enumerate(per_model):
        inst = np.zeros(count, api.IM_INSTANCE)
        inst["pos"] = rng.uniform(-args.box / 2, args.box / 2, (count, 3)).astype(np.float32)
        q = rng.normal(size=(count, 4))
        q /= np.sqrt((q ** 2).sum(1))[:, None]
        inst["rot"] = (q[:, :3] * np.sign(q[:, 3:4])).astype(np.float32)  # (w >= 0: the instance keeps xyz only)
        inst["scale"] = rng.uniform(0.5, 2.0, count).astype(np.float32)
        im.addModel([1e8, -1, -1, -1], [(0, 0), (0, -1), (0, -1), (0, -1), (0, -1)], 1.001, [3 * tris[k]])
        im.setInstances(k, inst)
    im.setOrigins(origins)
    out = {"instances": n, "box": args.box, "model_triangles": tris, "steps": args.steps, "fp32_ops_per_pair_assumed": FP32_OPS_PER_PAIR, "batches": {}}
    for n_rays in (int(x) for x in args.rays.split(",")):
        d = rng.normal(size=(n_rays, 3))
        d /= np.sqrt((d ** 2).sum(1))[:, None]
        rays = api.rays(np.tile(centre, (n_rays, 1)), d)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        rc.setInstancedModels(im, np.arange(len(shapes)), 100 + np.arange(len(shapes)))
        rc.reserve(n_rays, max(1024, 64 * n_rays))
        rc.castDevice(d_rays.data_ptr(), n_rays)
        cnt = rc.imCounts()
        if cnt["overflow"]:
            rc.reserve(n_rays, cnt["candidates"])
            rc.castDevice(d_rays.data_ptr(), n_rays)
            cnt = rc.imCounts()
        assert cnt["overflow"] == 0 and rc.counts()["overflow"] == 0, cnt

        def spans(cold):
            t = []
            for k in range(3 + args.steps):
                if cold:
                    scrub.fill_(float(k))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc.castDevice(d_rays.data_ptr(), n_rays)
                b.record()
                b.synchronize()
                if k >= 3:
                    t.append(a.elapsed_time(b) * 1e3)
            return {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}

        r = {"candidates": cnt["candidates"], "candidates_per_ray": cnt["candidates"] / n_rays, "warm": spans(False), "behind_1GiB_scrub": spans(True)}
        assert rc.imCounts() == cnt
        r["hits"] = int(rc.readImHits()["is_hit"].sum())
        r["pairs"] = n * n_rays
        for k in ("warm", "behind_1GiB_scrub"):
            r[k]["pairs_per_ns"] = r["pairs"] / (r[k]["median_us"] * 1e3)
            r[k]["assumed_fp32_tflops"] = r["pairs"] * FP32_OPS_PER_PAIR / (r[k]["median_us"] * 1e-6) / 1e12
        if args.plain:
            rc.setInstancedModels(None)
            r["detached_warm"] = spans(False)
        out["batches"][str(n_rays)] = r
    rc.setInstancedModels(None)
    im.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
