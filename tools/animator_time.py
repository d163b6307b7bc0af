#!/usr/bin/env python
"""Times a frame of Animators on the device: --instances Animators x 64 bones, two SAMPLE layers each, produced by a BLEND1D between two clips
(DESIGN.md §4.16's mode (a)), through
  i   the path without the node graph on the device: lmx_anim_eval_blend_instrs fed the same records from host arrays - the kernel and the
      whole call (two pageable uploads, the synchronise, the launch, up to the stream's end). The host-side node evaluation and the decode of
      the blend stack bytes that this path needs in front are NOT charged.
  ii  lmx_animators_set_inputs for all Animators + lmx_animators_update, up to the synchronise, with its kernels split out: Controller::update
      (k_animators_update), scan + pack, and the blend kernel (k_anim_blend_instrs, the same kernel as in i on the same records).
The two alternate inside one process, --rounds rounds of --steps calls each: every step runs ii, reads its records back (not timed) and
hands them to i. One JSON line: medians per mode and per round - the rounds of i against each other are the spread ii is held against.
Nothing is asserted here: `holds` states the two comparisons of DESIGN.md §4.18 for this run.

    python tools/animator_time.py [--instances 100000] [--steps 20] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumixengine_amd import api, scenes  # noqa: E402
from tests import controller_cases as K  # noqa: E402  (the writer of the compiled controller format)
from tools.ik_time import BONES, animations, skeleton  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.zeros(1, device="cuda")  # torch opens the device before the library does
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    sk = api.Skinning(ctx)
    s = skeleton()
    model = sk.addModel(s["parents"], s["bind"], s["first_nonroot"])
    mesh = sk.addMesh(*scenes.skinned_mesh(16, BONES, seed=6))
    n = args.instances
    sk.setInstances(np.full(n, model, np.uint32), np.full(n, mesh, np.uint32))
    sk.setModelPose(model, s["bind"])
    ids = [sk.addAnimation(a) for a in animations()]
    an = api.Animators(sk)
    rng = np.random.default_rng(3)
    for i, a in zip(ids, animations()):
        an.setRootMotion(i, np.cumsum(rng.uniform(-0.05, 0.05, size=(a["frame_count"] + 1, 3)), axis=0).astype(np.float32), None)
    ctl = an.addController(K.controller_bytes(("blend1d", [(0.0, 0), (1.0, 1)], K.inp(0)), [K.NUMBER], 2))
    an.setSlots(ctl, 0, ids)
    an.setAnimators(np.full(n, ctl, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(n, -1, np.int32))
    values = np.zeros(n, api.ANIMATOR_VALUE)
    values["type"] = api.VALUE_NUMBER
    kid = {k: api.KERNEL_NAMES.index(k) for k in ("anim_update", "animators_update", "animators_pack")}
    ctx.profile_enable(True)

    def frame_new(step):
        values["v"][:, 0] = rng.uniform(0.05, 0.95, n).astype(np.float32).view(np.uint32)  # what the game changed this frame: every Animator's input
        ctx.profile_reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        an.setInputs(0, n, values)
        an.update(1.0 / 60.0)
        b.record()
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e6
        k = {name: ctx.profile_get(i) for name, i in kid.items()}
        assert all(launches == 1 for (_, launches) in k.values()), k
        return [k["animators_update"][0] * 1e3, k["animators_pack"][0] * 1e3, k["anim_update"][0] * 1e3, a.elapsed_time(b) * 1e3, wall]

    def call_old(first, rec):
        ctx.profile_reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        ctx.check(sk.lib.lmx_anim_eval_blend_instrs(ctx.h, n, api._ptr(first), api._ptr(rec)))
        b.record()
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e6
        ms, launches = ctx.profile_get(kid["anim_update"])
        assert launches == 1, launches
        return [ms * 1e3, a.elapsed_time(b) * 1e3, wall]

    for step in range(3):  # warm-up of both paths
        frame_new(step)
        first, rec = an.readInstrs()
        call_old(first, rec)
    new, old, same = [], [], True
    for r in range(args.rounds):
        rn, ro = [], []
        for step in range(args.steps):
            rn.append(frame_new(step))
            first, rec = an.readInstrs()
            assert len(rec) == 2 * n
            pose_new = [sk.readRelativePose(i) for i in (0, n - 1)] if step == 0 else None
            ro.append(call_old(first, np.ascontiguousarray(rec)))
            if pose_new is not None:
                pose_old = [sk.readRelativePose(i) for i in (0, n - 1)]
                same = same and all(np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(pose_new, pose_old))
        new.append(rn)
        old.append(ro)

    def stats(t, names):
        t = np.array(t)  # [round, step, column]
        return {name: {"median_us": float(np.median(t[:, :, k])), "min_us": float(t[:, :, k].min()), "max_us": float(t[:, :, k].max()),
                       "round_medians_us": [float(np.median(t[r, :, k])) for r in range(t.shape[0])]} for k, name in enumerate(names)}

    out = {"instances": n, "bones": BONES, "steps": args.steps, "rounds": args.rounds, "poses_equal_bitwise": bool(same),
           "i_eval_blend_instrs_from_host_records": stats(old, ("blend_kernel", "stream_span", "host_wall")),
           "ii_set_inputs_and_animators_update": stats(new, ("controller_update_kernel", "scan_and_pack", "blend_kernel", "stream_span", "host_wall"))}
    oi, ni = out["i_eval_blend_instrs_from_host_records"], out["ii_set_inputs_and_animators_update"]
    # what the feature is held to, as stated: (ii)'s blend kernel within (i)'s round-to-round spread - between the lowest and the highest round median
    # of (i) - and (ii)'s whole frame not longer than (i)'s whole call, with (i)'s own spread in this run as the margin
    rk, rw = oi["blend_kernel"]["round_medians_us"], oi["host_wall"]["round_medians_us"]
    out["holds"] = {
        "blend_kernel_of_ii_within_the_round_to_round_spread_of_i": bool(min(rk) <= ni["blend_kernel"]["median_us"] <= max(rk)),
        "blend_kernel_of_ii_minus_nearest_round_median_of_i_us": float(ni["blend_kernel"]["median_us"] - min(rk, key=lambda x: abs(x - ni["blend_kernel"]["median_us"]))),
        "whole_frame_of_ii_not_longer_than_the_whole_call_of_i": bool(ni["host_wall"]["median_us"] <= oi["host_wall"]["median_us"] + (max(rw) - min(rw))),
        "spread_of_i_blend_kernel_us": max(rk) - min(rk), "spread_of_i_host_wall_us": max(rw) - min(rw)}
    ctx.close()
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
