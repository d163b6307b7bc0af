"""Instanced-model workload: 10 M instances over 16 models, camera inside the field, a main view + 4 shadow cascades per
frame. Times lmx_im_run per view (host clock around the run + a stream synchronise, median of --steps), warm (back to back) and cold (a
scrub larger than the 256 MiB L3 between runs), and prints one JSON line with the algorithmic bytes of the split layout:

  read   20 B per instance of a near cell (pos_scale 16 + lod 4; far cells: 0) in k_im_count, 1/8 B of mask per instance in k_im_emit,
         36 B per emitting instance (lod 4 + pos_scale 16 + rot 16) in k_im_emit
  write  4 B of LOD per instance of a near cell (non-shadow views), 1/8 B of mask per instance, 32 B per emitted record

    python tools/im_time.py [--instances 10000000] [--models 16] [--steps 20] [--views 5]
(rocprofv3 --kernel-trace --stats around it, in a run of its own, gives the two kernels' own times.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BPS = 8.0e12  # MI355X HBM3E


def scene(api, n_total, n_models, seed=1):
    rng = np.random.default_rng(seed)
    im_models = []
    per = n_total // n_models
    for k in range(n_models):
        inst = np.zeros(per, api.IM_INSTANCE)
        inst["pos"][:, 0] = rng.uniform(-500, 500, per)
        inst["pos"][:, 1] = rng.uniform(0, 2, per)
        inst["pos"][:, 2] = rng.uniform(-500, 500, per)
        q = rng.normal(size=(per, 4)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        inst["rot"] = q[:, :3]
        inst["lod"] = rng.uniform(0, 4, per).astype(np.float32)
        inst["scale"] = rng.uniform(0.5, 2.0, per).astype(np.float32)
        im_models.append(inst)
    origins = [[1000.0 * (k % 4) - 1500.0, 0.0, 1000.0 * (k // 4) - 1500.0] for k in range(n_models)]
    return im_models, origins


def views(api, cam):
    d = np.array([np.sin(0.3), -0.15, -np.cos(0.3)], np.float32)
    out = [(api.frustum_perspective(cam, d, np.array([0, 1, 0], np.float32), float(np.deg2rad(70)), 16 / 9, 0.1, 2000.0), False)]
    light = np.array([0.3, -0.8, 0.5], np.float32)
    light /= np.linalg.norm(light)
    for k in range(4):
        size = 20.0 * (3 ** k)
        out.append((api.frustum_ortho(np.asarray(cam, np.float64) - 200 * light.astype(np.float64), light, np.array([0, 0, 1], np.float32), size, size, 0.0, 400.0), True))
    return out


def algorithmic_bytes(n_total, n_near, emitting, emitted, shadow):
    """(bytes read, bytes written) of one view run in the split layout (module docstring)"""
    read = 20 * n_near + n_total / 8 + 36 * emitting
    write = (0 if shadow else 4 * n_near) + n_total / 8 + 32 * emitted
    return read, write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=10_000_000)
    ap.add_argument("--models", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--no-scrub", action="store_true", help="rehearsal on the simulated device: no cold leg")
    a = ap.parse_args()
    from lumixengine_amd import api

    torch = None
    if not a.no_scrub:  # torch's device first, the library on its stream (as tools/run_workload.py)
        import torch

        scrub = torch.zeros(1 << 29, dtype=torch.int32, device="cuda")  # 2 GiB, read between cold runs: larger than the 256 MiB L3
    ctx = api.Context(0)
    if torch is not None:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    im = api.InstancedModels(ctx)
    models, origins = scene(api, a.instances, a.models)
    t = time.perf_counter()
    for inst in models:
        m = im.addModel([400.0, 3600.0, 22500.0, 90000.0], [(0, 0), (1, 1), (2, 2), (3, 3), (0, -1)], 1.0, [24, 18, 12, 6])
        im.setInstances(m, inst)
    ctx.synchronize()
    build_s = time.perf_counter() - t
    im.setOrigins(origins)
    cam = (0.0, 8.0, 0.0)
    vs = views(api, cam)[: a.views]
    out = {"instances": a.instances, "models": a.models, "grid_build_s_all_models": build_s, "launches_per_run": 2, "views": []}
    n_total = a.instances
    for vi, (fr, shadow) in enumerate(vs):
        view = api.im_view(cam, 1.0, 0.0, is_shadow=shadow)  # time_delta 0: every step does the same work
        for _ in range(3):
            im.run(view, fr, vi)
        ctx.synchronize()
        warm, cold = [], []
        for _ in range(a.steps):
            t = time.perf_counter()
            im.run(view, fr, vi)
            ctx.synchronize()
            warm.append(time.perf_counter() - t)
        for _ in range(a.steps if torch is not None else 0):
            scrub.sum()
            torch.cuda.synchronize()
            t = time.perf_counter()
            im.run(view, fr, vi)
            ctx.synchronize()
            cold.append(time.perf_counter() - t)
        c = im.counts(vi)
        emitted = int(c["bin_count"].sum())
        # instances of near cells / emitting instances: from the device's own grids and counts (cells' verdicts are per block: the
        # host restates them with the oracle's cell pass)
        from tests import im_oracle as O

        n_near = 0
        for m in range(a.models):
            g = im.readGrid(m)
            gd = {"count": g["cells"]["instance_count"], "cmin": g["cells"]["min"], "cmax": g["cells"]["max"]}
            v = O.cell_verdicts(gd, origins[m], 1.0, np.sqrt(np.float32(90000.0)), cam, fr)
            n_near += int(g["cells"]["instance_count"][v > 0].sum())
        emitting = int(np.count_nonzero(im.readRecords(vi)["lod"] >= 0))  # an instance's first record carries w = frac >= 0, a second one frac - 1 < 0
        rd, wr = algorithmic_bytes(n_total, n_near, emitting, emitted, shadow)
        w, cd = float(np.median(warm)), float(np.median(cold)) if cold else float("nan")
        out["views"].append({"view": "main" if not shadow else f"cascade{vi}", "warm_us": w * 1e6, "cold_us": cd * 1e6, "emitted": emitted, "emitting_instances": emitting, "near_instances": n_near,
                             "bytes_read": rd, "bytes_written": wr, "frac_of_8TBps_cold": (rd + wr) / PEAK_BPS / cd, "frac_of_8TBps_warm": (rd + wr) / PEAK_BPS / w})
    print(json.dumps(out))
    im.close()
    ctx.close()


if __name__ == "__main__":
    main()
