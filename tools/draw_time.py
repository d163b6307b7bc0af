#!/usr/bin/env python
"""Times the device chain lmx_keys_run -> lmx_keys_sort -> lmx_draw_run on the dense 10 M workload of tools/run_workload.py (about 1 M
visible): device spans between events on the context's stream, warm and behind a 1 GiB scrub of the caches, one JSON line.

    python tools/draw_time.py --steps 20 [--entities 10000000] [--batches 8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--entities", type=int, default=10_000_000)
    ap.add_argument("--batches", type=int, default=8)
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api, scenes

    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    sc = scenes.cull_scene(args.entities, 5000.0, seed=2)
    n = len(sc["entity"])
    cs = api.CullingSystem(ctx)
    cs.build(sc["entity"], sc["type"], sc["pos"], sc["radius"])
    fr = api.viewport_frustum()
    ks = scenes.keys_scene(n, sc["type"], seed=12, max_sort_key=255)
    dt = scenes.draw_tables(ks, n, seed=14, extent=5000.0)
    tr = scenes.random_transforms(np.random.default_rng(15), n, 1.0)
    tr["pos"] = sc["pos"]
    sk = api.SortKeys(ctx)
    sk.setModels(ks["models"], ks["mesh_types"])
    sk.setInstances(ks["model"], ks["material_offset"], ks["mesh_materials"], ks["lod"], ks["flags"], ks["dirty"], ks["pose_frame"])
    sk.setDecals(n, ks["decal_key"], ks["decal_layer"], ks["curve_key"], ks["curve_layer"])
    sk.setPositions(sc["pos"])
    dc = api.DrawCommands(ctx)
    dc.setMeshes(dt["mesh_lod"])
    dc.setMaterialIndices(dt["material_index"])
    dc.setTransforms(tr)
    dc.setPrevTransforms(dt["prev"])
    dc.setBones(dt["bones_handle"], dt["bones_offset"])
    dc.setDecals(n, dt["half_extents"], dt["uv_scale"], dt["decal_material"], dt["curve_half_extents"], dt["curve_uv_scale"], dt["curve_bezier"], dt["curve_material"])
    dv = api.draw_view(frustum=fr, bucket_depth_sorted=ks["bucket_depth_sorted"])
    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB

    def frame(f, cold):
        cs.cull(fr)
        kv = api.keys_view(layer_to_bucket=ks["layer_to_bucket"], bucket_depth_sorted=ks["bucket_depth_sorted"], frame_number=100 + f)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        if cold:
            scrub.add_(1.0)
        e[0].record()
        sk.run(kv, 255)
        e[1].record()
        sk.sort()
        e[4].record()
        if cold:
            scrub.add_(1.0)
        e[2].record()
        dc.run(dv, args.batches)
        e[3].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]) * 1e3, e[2].elapsed_time(e[3]) * 1e3, e[0].elapsed_time(e[4]) * 1e3

    for f in range(3):
        frame(f, False)
    out = {"entities": n, "batches": args.batches}
    for name, cold in (("warm", False), ("cold", True)):
        t = np.array([frame(10 + f, cold) for f in range(args.steps)])
        out[name] = {"keys_run_us": float(np.median(t[:, 0])), "draw_run_us": float(np.median(t[:, 1])), "draw_run_min_us": float(t[:, 1].min())}
        out[name]["keys_run_sort_us"] = float(np.median(t[:, 2]))  # lmx_keys_run + lmx_keys_sort (the sort reads its count on the host: the span holds that gap)
        out[name]["draw_to_keys_run"] = out[name]["draw_run_us"] / out[name]["keys_run_us"]
        out[name]["draw_to_keys_run_sort"] = out[name]["draw_run_us"] / out[name]["keys_run_sort_us"]
    out["keys_counts"] = sk.counts()
    out["draw_counts"] = dc.counts()
    kinds, cnt = np.unique(dc.readRuns()["kind"], return_counts=True)
    out["runs_by_kind"] = {int(k): int(c) for k, c in zip(kinds, cnt)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
