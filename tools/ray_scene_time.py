#!/usr/bin/env python
"""Times the whole castRay on the device: the span of lmx_rays_cast_device's launches with the scene of tools/ray_im_time.py (--instances
instances of four instanced models around (1e6, 50, -1e6), no model instance), one --terrain x --terrain R16 terrain under it and
--geometries procedural geometries of about 1 k triangles (the 1 k sphere, scattered), for batches of 1, 1024 and 65 536 rays from the
cube's centre. Median of --steps, warm (back to back) and behind a 1 GiB scrub of the caches; one JSON line. --plain 1 adds the span of the
same cast with both tables cleared (the launch chain of before: instanced models + model instances).

    python tools/ray_scene_time.py --steps 20 [--instances 1000000] [--rays 1,1024,65536]

The rays are in device memory before the span starts; no count reaches the host inside it. No bar is fixed. Per-kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run (tools/gpu_cases/rays_scene.sh).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--instances", type=int, default=1_000_000)
    ap.add_argument("--rays", default="1,1024,65536")
    ap.add_argument("--box", type=float, default=1000.0)
    ap.add_argument("--terrain", type=int, default=2048)
    ap.add_argument("--geometries", type=int, default=64)
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
    # entity 0: nobody; 1: the terrain, its corner below the cube; 2 ...: the procedural geometries
    cell = args.box / args.terrain
    tr = np.zeros(2 + args.geometries, api.TRANSFORM)
    tr["rot"][:, 3], tr["scale"] = 1, 1
    tr["pos"][1] = centre + [-args.box / 2, -args.box / 2, -args.box / 2]
    tr["pos"][2:] = centre + rng.uniform(-args.box / 4, args.box / 4, (args.geometries, 3))
    q = rng.normal(size=(args.geometries, 4)).astype(np.float32)
    tr["rot"][2:] = q / np.sqrt((q.astype(np.float64) ** 2).sum(1))[:, None].astype(np.float32)
    tr["scale"][2:] = rng.uniform(5, 40, (args.geometries, 3)).astype(np.float32)
    api.DrawCommands(ctx).setTransforms(tr)
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
    rc.setInstances(np.full(1, -1, np.int32), np.zeros(1, np.uint8))
    im = api.InstancedModels(ctx)
    origins = centre + rng.uniform(-5, 5, (len(shapes), 3))
    per_model = [n // len(shapes)] * (len(shapes) - 1) + [n - (len(shapes) - 1) * (n // len(shapes))]
    for k, count in enumerate(per_model):
        inst = np.zeros(count, api.IM_INSTANCE)
        inst["pos"] = rng.uniform(-args.box / 2, args.box / 2, (count, 3)).astype(np.float32)
        q = rng.normal(size=(count, 4))
        q /= np.sqrt((q ** 2).sum(1))[:, None]
        inst["rot"] = (q[:, :3] * np.sign(q[:, 3:4])).astype(np.float32)
        inst["scale"] = rng.uniform(0.5, 2.0, count).astype(np.float32)
        im.addModel([1e8, -1, -1, -1], [(0, 0), (0, -1), (0, -1), (0, -1), (0, -1)], 1.001, [3 * tris[k]])
        im.setInstances(k, inst)
    im.setOrigins(origins)
    # rolling hills up to a fifth of the cube's height
    gx, gz = np.meshgrid(np.arange(args.terrain), np.arange(args.terrain))
    heightmap = ((np.sin(gx / 97.0) * np.cos(gz / 131.0) * 0.5 + 0.5) * 65535).astype(np.uint16)
    terrains = [{"entity": 1, "scale": (cell, args.box / 5, cell), "heightmap": heightmap}]
    pos, idx = shapes[0]
    geoms = [{"entity": 2 + g, "aabb_min": [-1.001] * 3, "aabb_max": [1.001] * 3, "vertex_data": pos, "stride": 12, "indices": idx} for g in range(args.geometries)]
    out = {"instances": n, "box": args.box, "terrain": args.terrain, "geometries": args.geometries, "geometry_triangles": tris[0], "steps": args.steps, "batches": {}}
    for n_rays in (int(x) for x in args.rays.split(",")):
        d = rng.normal(size=(n_rays, 3))
        d /= np.sqrt((d ** 2).sum(1))[:, None]
        rays = api.rays(np.tile(centre, (n_rays, 1)), d)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        rc.setInstancedModels(im, np.arange(len(shapes)), 100 + np.arange(len(shapes)))
        rc.setProceduralGeometries(geoms)
        rc.setTerrains(terrains)
        rc.reserve(n_rays, max(1024, 64 * n_rays))
        rc.castDevice(d_rays.data_ptr(), n_rays)
        need = max(rc.imCounts()["candidates"], rc.sceneCounts()["candidates"], rc.counts()["candidates"])
        if rc.counts()["overflow"]:
            rc.reserve(n_rays, need)
            rc.castDevice(d_rays.data_ptr(), n_rays)
        assert rc.counts()["overflow"] == 0, rc.counts()

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

        r = {"im_candidates": rc.imCounts()["candidates"], "pg_candidates": rc.sceneCounts()["candidates"], "warm": spans(False), "behind_1GiB_scrub": spans(True)}
        hits = rc.readSceneHits()
        r["hits_by_component"] = np.bincount(hits["component"], minlength=5).tolist()
        r["terrain_hits"] = int(rc.readTerrainHits()["is_hit"].sum())
        if args.plain:
            rc.setProceduralGeometries([])
            rc.setTerrains([])
            r["tables_cleared_warm"] = spans(False)
            r["tables_cleared_behind_1GiB_scrub"] = spans(True)
        out["batches"][str(n_rays)] = r
    rc.setProceduralGeometries([])
    rc.setTerrains([])
    rc.setInstancedModels(None)
    im.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
