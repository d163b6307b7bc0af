#!/usr/bin/env python
"""Times the pose processor on the device: the span of lmx_poses_run's three launches (HIP events on the context's stream, the library's own
profile slots) over 1 %, 10 % and 100 % of 100 k instances x 64 bones listed, next to lmx_skin_run's pose kernel computing the dual
quaternions of EVERY instance (lmx_skin_enable_dual_quats) and without them. Median of --steps, one JSON line.

    python tools/pose_time.py --steps 20 [--instances 100000] [--bones 64]

The list is a caller-given one (lmx_poses_run_list: the same pass as lmx_poses_run, whose list is wherever the cull left the visible
instances - no order either way); the upload of the list lies outside the timed span.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
BYTES_PER_BONE = 56 + 32  # absolute pose 28 B + inverse bind 28 B read, DualQuat written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--instances", type=int, default=100_000)
    ap.add_argument("--bones", type=int, default=64)
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api, scenes

    n, nb = args.instances, args.bones
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    s = scenes.skeleton(nb, seed=4)
    verts, skin = scenes.skinned_mesh(8, nb, seed=6)  # lmx_skin_run skins vertices too: next to nothing here
    pos, rot = scenes.relative_poses(n, nb, seed=5)
    sk = api.Skinning(ctx)
    model, mesh = sk.addModel(s["parents"], s["bind"], s["first_nonroot"]), sk.addMesh(verts, skin)
    sk.setInstances(np.full(n, model, np.uint32), np.full(n, mesh, np.uint32))
    d_pos, d_rot = torch.from_numpy(pos.reshape(-1)).cuda(), torch.from_numpy(rot.reshape(-1)).cuda()
    sk.setPoseSourceDevice(d_pos.data_ptr(), d_rot.data_ptr(), n * nb)  # relative poses for every run, absolute ones into the library's arrays
    ctx.profile_enable(True)

    def spans(kernel, call, before=lambda: None):
        for _ in range(3):
            before()
            call()
        t = []
        for _ in range(args.steps):
            before()
            ctx.profile_reset()
            call()
            t.append(ctx.profile_get(kernel)[0] * 1e3)
        return {"median_us": float(np.median(t)), "min_us": float(np.min(t))}

    out = {"instances": n, "bones": nb, "steps": args.steps}
    K_POSE_PALETTE = api.KERNEL_NAMES.index("pose_palette")
    sk.enableDualQuats(False)
    out["skin_pose_kernel"] = spans(K_POSE_PALETTE, sk.run)
    sk.enableDualQuats(True)
    out["skin_pose_kernel_with_dual_quats_of_all"] = spans(K_POSE_PALETTE, sk.run)
    out["dual_quats_of_all_us"] = out["skin_pose_kernel_with_dual_quats_of_all"]["median_us"] - out["skin_pose_kernel"]["median_us"]

    pp = api.PoseProcessor(ctx)
    pp.setInstances(np.arange(n, dtype=np.int32))  # entity i carries instance i
    rng = np.random.default_rng(7)
    for share in (0.01, 0.1, 1.0):
        listed = rng.permutation(n)[: max(int(n * share), 1)].astype(np.int32)
        r = spans(api.K_POSE_SLICES, lambda: pp.runList(listed), lambda: pp.beginFrame(1, 0))
        cnt = pp.counts()
        assert cnt == {"instances": len(listed), "bytes": 32 * nb * len(listed), "skipped": 0, "overflow": 0}, cnt
        r["listed"] = len(listed)
        r["bytes"] = BYTES_PER_BONE * nb * len(listed)
        r["share_of_8_TB_per_s"] = r["bytes"] / (r["median_us"] * 1e-6) / HBM_BYTES_PER_S
        # the slices hold what the skin run's palette holds for the same instances
        _, off = pp.readSlices()
        buf = pp.readBuffer()
        for e in listed[:5]:
            assert buf[off[e] : off[e] + 32 * nb].tobytes() == sk.readDualQuats(int(e)).tobytes(), int(e)
        out[f"poses_run_{share:g}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
