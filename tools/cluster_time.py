#!/usr/bin/env python
"""Times fillClusters on the device: the span of lmx_clusters_run's four launches (stream events around the call) over the LOCAL_LIGHT
list a cull left on the device, on a 1920 x 1080 view (30 x 17 x 16 clusters) with 1 k, 10 k and 100 k visible lights of radii 5-50
scattered through the view's volume of a 3e4 scene. Median of --steps, warm (back to back) and behind a 1 GiB scrub of the caches;
one JSON line.

    python tools/cluster_time.py --steps 20 [--lights 1000,10000,100000]

The cull and the gather of its shard windows into one list per type (once per cull result) lie outside the timed span; the list's
length never reaches the host inside it. Algorithmic bytes: per listed light its 4 B id, the 56 B transform, the 32 B table record
and the 4 B atlas slot read, the 64 B record written; 4 B per map entry; 16 B per cluster. Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool (tools/gpu_cases/clusters.sh).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SCENE = 3.0e4
W, H = 1920, 1080
TYPE_LOCAL_LIGHT = 2


def visible_lights(rng, n, fov=np.deg2rad(60.0), far=1.0e4):
    """n positions (relative to a camera looking down -z) inside the view's pyramid, depth uniform up to the clusters' far plane, and radii 5-50."""
    z = -rng.uniform(1.0, min(far, SCENE), n)
    half_y = np.tan(fov / 2) * -z
    half_x = half_y * (W / H)
    pos = np.stack([rng.uniform(-1, 1, n) * half_x, rng.uniform(-1, 1, n) * half_y, z], axis=1)
    return pos, rng.uniform(5.0, 50.0, n).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lights", default="1000,10000,100000")
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api

    cam = np.array([1.0e6, 50.0, -1.0e6])
    frustum = api.viewport_frustum(w=W, h=H, pos=cam)
    view = api.cluster_view(cam, frustum, W, H)
    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB
    out = {"viewport": [W, H], "steps": args.steps, "sizes": {}}
    for n in (int(x) for x in args.lights.split(",")):
        rng = np.random.default_rng(n)
        ctx = api.Context(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        rel, radius = visible_lights(rng, n)
        tr = np.zeros(n, api.TRANSFORM)
        tr["pos"], tr["rot"], tr["scale"] = cam + rel, (0, 0, 0, 1), 1
        lights = np.zeros(n, api.POINT_LIGHT)
        lights["color"], lights["intensity"], lights["range"], lights["fov"] = 1, 2, radius, 1
        cs = api.CullingSystem(ctx)
        cs.build(np.arange(n, dtype=np.int32), np.full(n, TYPE_LOCAL_LIGHT, np.uint8), tr["pos"], radius)
        api.DrawCommands(ctx).setTransforms(tr)
        cf = api.ClusterFiller(ctx)
        cf.setLights(lights)
        cf.reserve(n, 1 << 22)
        cs.cull(frustum, TYPE_LOCAL_LIGHT, view=0)
        cf.run(view, cull_view=0)  # (also gathers the cull's shard windows, once per cull result)
        cnt = cf.counts()
        if cnt["overflow"]:
            cf.reserve(max(n, cnt["lights"]), cnt["map_entries"])
            cf.run(view, cull_view=0)
            cnt = cf.counts()
        assert cnt["overflow"] == 0, cnt

        def spans(cold):
            t = []
            for k in range(3 + args.steps):
                if cold:
                    scrub.fill_(float(k))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                cf.run(view, cull_view=0)
                b.record()
                b.synchronize()
                if k >= 3:
                    t.append(a.elapsed_time(b) * 1e3)
            return {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}

        r = {"listed": cnt["lights"], "map_entries": cnt["map_entries"], "warm": spans(False), "behind_1GiB_scrub": spans(True)}
        assert cf.counts() == cnt
        clusters, size = cf.readClusters()
        r["lights_per_cluster_max"] = int(clusters["lights_count"].max())
        r["algorithmic_bytes"] = cnt["lights"] * (4 + 56 + 32 + 4 + 64) + 4 * cnt["map_entries"] + 16 * len(clusters)
        r["range_tests"] = cnt["lights"] * len(clusters) * 2  # the count and the fill step each test every light against every cluster
        for k in ("warm", "behind_1GiB_scrub"):
            r[k]["share_of_8_TB_per_s"] = r["algorithmic_bytes"] / (r[k]["median_us"] * 1e-6) / HBM_BYTES_PER_S
            r[k]["range_tests_per_ns"] = r["range_tests"] / (r[k]["median_us"] * 1e3)
        out["sizes"][str(n)] = r
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
