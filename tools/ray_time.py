#!/usr/bin/env python
"""Times batched ray casts on the device: the span of lmx_rays_cast_device's launches (two fills, broad phase, narrow phase, resolve,
write-out; stream events around the call) over --instances model instances of four models (a 1 k, a 4 k and a 10 k triangle sphere and a
5 k triangle skinned one carried by 1024 of the instances) scattered through a --box cube, for batches of 1, 1024 and 65 536 rays from the
cube's centre. Median of --steps, warm (back to back) and behind a 1 GiB scrub of the caches; one JSON line.

    python tools/ray_time.py --steps 20 [--instances 1000000] [--rays 1,1024,65536]

The rays are in device memory before the span starts; the candidate count never reaches the host inside it. Algorithmic bytes: per
(ray, entity) pair tested 61 B of the entity (transform, model, flags) per RAY_BROAD_RAYS rays + 48 B of the ray per RAY_BLOCK entities;
per candidate 48 B written and read; per candidate triangle its three indices and 36 B of positions, + 24 B per skinned corner. Per-kernel
times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (tools/gpu_cases/rays.sh).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
N_SKINNED = 1024
N_BONES = 32


def sphere(n_lat, n_lon, radius=1.0):
    """a UV sphere of 2 * n_lon * (n_lat - 1) triangles, uint16 indices where they fit"""
    lat = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.cos(lat), np.ones(n_lon)), np.outer(np.sin(lat), np.sin(lon))], -1).reshape(-1, 3)
    pos = np.concatenate([[[0, 1, 0]], ring, [[0, -1, 0]]]).astype(np.float32) * np.float32(radius)
    tris = []
    at = lambda i, j: 1 + i * n_lon + j % n_lon
    for j in range(n_lon):
        tris.append((0, at(0, j + 1), at(0, j)))
        tris.append((len(pos) - 1, at(n_lat - 2, j), at(n_lat - 2, j + 1)))
        for i in range(n_lat - 2):
            tris += [(at(i, j), at(i, j + 1), at(i + 1, j)), (at(i, j + 1), at(i + 1, j + 1), at(i + 1, j))]
    idx = np.array(tris).reshape(-1)
    return pos, idx.astype(np.uint16 if len(pos) < 65536 else np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--instances", type=int, default=1_000_000)
    ap.add_argument("--rays", default="1,1024,65536")
    ap.add_argument("--box", type=float, default=1000.0)
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api

    n = args.instances
    rng = np.random.default_rng(7)
    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB (torch opens the device before the library does)
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    centre = np.array([1.0e6, 50.0, -1.0e6])
    tr = np.zeros(n, api.TRANSFORM)
    tr["pos"] = centre + rng.uniform(-args.box / 2, args.box / 2, (n, 3))
    q = rng.normal(size=(n, 4)).astype(np.float32)
    tr["rot"] = q / np.sqrt((q.astype(np.float64) ** 2).sum(1))[:, None].astype(np.float32)
    tr["scale"] = rng.uniform(0.5, 2.0, (n, 3)).astype(np.float32)
    api.DrawCommands(ctx).setTransforms(tr)
    # the skinned model's skeleton: a chain, every instance in its bind pose (the palettes are read all the same)
    sk = api.Skinning(ctx)
    bind = np.zeros(N_BONES, api.LOCAL_RIGID)
    bind["rot"][:, 3] = 1
    smodel = sk.addModel(np.arange(-1, N_BONES - 1), bind, 1)
    tiny = sk.addMesh(np.zeros((3, 3), np.float32), np.zeros(3, api.SKIN))  # the ray caster holds its own copy of the geometry
    sk.setInstances(np.full(N_SKINNED, smodel), np.full(N_SKINNED, tiny))
    rel_rot = np.zeros((N_SKINNED * N_BONES, 4), np.float32)
    rel_rot[:, 3] = 1
    sk.uploadPoses(np.zeros((N_SKINNED * N_BONES, 3), np.float32), rel_rot)
    sk.run()
    rc = api.RayCaster(ctx)
    shapes = [sphere(23, 23), sphere(46, 45), sphere(72, 70), sphere(51, 50)]
    models = np.zeros(len(shapes), api.RAY_MODEL)
    tris = []
    for k, (pos, idx) in enumerate(shapes):
        skin = None
        if k == 3:
            skin = np.zeros(len(pos), api.SKIN)
            skin["indices"][:, 0], skin["indices"][:, 1] = rng.integers(0, N_BONES, len(pos)), rng.integers(0, N_BONES, len(pos))
            skin["weights"][:, 0], skin["weights"][:, 1] = 0.75, 0.25
        models[k]["first_mesh"], models[k]["mesh_count"], models[k]["ready"] = rc.addMesh(pos, idx, skin), 1, 1
        models[k]["aabb_min"], models[k]["aabb_max"], models[k]["origin_radius"] = -1.001, 1.001, 1.001
        tris.append(len(idx) // 3)
    rc.setModels(models)
    model = rng.integers(0, 3, n).astype(np.int32)
    skin_of_entity = np.full(n, -1, np.int32)
    chosen = rng.choice(n, N_SKINNED, replace=False)
    model[chosen], skin_of_entity[chosen] = 3, np.arange(N_SKINNED)
    api.PoseProcessor(ctx).setInstances(skin_of_entity)
    rc.setInstances(model, np.full(n, api.RAY_INSTANCE_ENABLED | api.RAY_INSTANCE_VALID, np.uint8))
    out = {"instances": n, "box": args.box, "model_triangles": tris, "steps": args.steps, "batches": {}}
    for n_rays in (int(x) for x in args.rays.split(",")):
        d = rng.normal(size=(n_rays, 3))
        d /= np.sqrt((d ** 2).sum(1))[:, None]
        rays = api.rays(np.tile(centre, (n_rays, 1)), d)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        rc.reserve(n_rays, max(1024, 64 * n_rays))
        rc.castDevice(d_rays.data_ptr(), n_rays)
        cnt = rc.counts()
        if cnt["overflow"]:
            rc.reserve(n_rays, cnt["candidates"])
            rc.castDevice(d_rays.data_ptr(), n_rays)
            cnt = rc.counts()
        assert cnt["overflow"] == 0, cnt

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
        assert rc.counts() == cnt
        cand = rc.readCandidates(cnt["candidates"])
        hits = rc.readHits()
        r["hits"] = int(hits["is_hit"].sum())
        per_model = np.bincount(cand["model"], minlength=len(shapes))
        r["candidate_triangles"] = int(sum(int(per_model[k]) * tris[k] for k in range(len(shapes))))
        r["pairs"] = n * n_rays
        pair_bytes = r["pairs"] * (61 / api.RAY_BROAD_RAYS + 48 / api.RAY_BLOCK)
        tri_bytes = sum(int(per_model[k]) * tris[k] * (3 * shapes[k][1].dtype.itemsize + 36 + (72 if k == 3 else 0)) for k in range(len(shapes)))
        r["algorithmic_bytes"] = int(pair_bytes + tri_bytes + 2 * 48 * cnt["candidates"] + 24 * n_rays)
        for k in ("warm", "behind_1GiB_scrub"):
            r[k]["share_of_8_TB_per_s"] = r["algorithmic_bytes"] / (r[k]["median_us"] * 1e-6) / HBM_BYTES_PER_S
            r[k]["pairs_per_ns"] = r["pairs"] / (r[k]["median_us"] * 1e3)
        out["batches"][str(n_rays)] = r
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
