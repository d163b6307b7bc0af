#!/usr/bin/env python
"""Times the Animator pose work on the device: --instances Animators x 64 bones, two SAMPLE layers each, through
  a_old  lmx_anim_eval_blend_stacks (k_anim_blend_stack),
  a_new  the same programs through lmx_anim_eval_blend_instrs (no IK in the call),
  b      + two 3-bone IK chains per instance,
  c      + one 16-bone IK chain per instance.
The four alternate inside one process, --rounds rounds of --steps calls each; per call the kernel's time (the library's event pair around
the launch), the stream span of the whole call (both uploads + the kernel) and the host's wall time up to the synchronise. One JSON line:
medians per mode and per round - the rounds of a_old against each other are the run-to-run spread a_new is held against.

    python tools/ik_time.py [--instances 100000] [--steps 20] [--rounds 3]
    python tools/ik_time.py --reference [--sample 512]    # one-thread CPU time of the reference's evalIK for b and c (needs the reference tree, no GPU)

--reference cuts evalIK out of the reference tree as tests/test_ik_oracle_vs_ref.py does, runs it on the poses the two SAMPLE layers leave
for --sample of the instances (the CPU oracle samples them) and scales to --instances. No bar is fixed.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumixengine_amd import api, scenes  # noqa: E402

BONES = 64
ONE_SECOND = 1 << 15
CHAINS = {"b": [(31, 3), (39, 3)], "c": [(23, 16)]}  # (leaf bone, bones_count)


def skeleton():
    """a 24-bone spine and five 8-bone limbs hanging off bone 8: a 16-bone chain up the spine, 3-bone chains at two limb ends"""
    rng = np.random.default_rng(7)
    parents = np.arange(-1, BONES - 1).astype(np.int16)
    for first in range(24, BONES, 8):
        parents[first] = 8
    rel = np.zeros(BONES, api.LOCAL_RIGID)
    rel["pos"] = rng.uniform(-0.3, 0.3, size=(BONES, 3)).astype(np.float32)
    rel["rot"] = scenes.random_unit_quats(rng, BONES)
    return {"parents": parents, "bind": rel, "first_nonroot": 1}


def programs(n, mode, ids, seed=11):
    """BLEND_INSTR [n, k]: two SAMPLE layers, then the mode's IK instructions"""
    rng = np.random.default_rng(seed)
    chains = CHAINS.get(mode, [])
    ins = np.zeros((n, 2 + len(chains)), api.BLEND_INSTR)
    ins["leaf_bone"] = api.BONE_NONE
    for layer, (weight, length) in enumerate(((1.0, 30), (0.5, 12))):
        ins["op"][:, layer], ins["animation"][:, layer], ins["weight"][:, layer], ins["looped"][:, layer] = api.BLEND_SAMPLE_OP, ids[layer], weight, 1
        ins["time"][:, layer] = rng.integers(0, length * ONE_SECOND // 30, n)
    for k, (leaf, count) in enumerate(chains):
        c = ins[:, 2 + k]
        c["op"], c["alpha"], c["leaf_bone"], c["bones_count"] = api.BLEND_IK_OP, 1.0, leaf, count
        c["target"] = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    return ins


def animations():
    return [scenes.animation(BONES, 30, 30.0, seed=61), scenes.animation(BONES, 12, 30.0, seed=62, root_motion=False)]


def reference(args):
    from oracle import pyoracle
    from tests import test_ik_oracle_vs_ref as R

    if not os.path.exists(pyoracle.ORACLE_SO):
        pyoracle.build()
    oracle = pyoracle.Oracle("port")
    d = tempfile.mkdtemp(prefix="ik_time_ref_")
    exe = R.build_harness(d)
    s, anims = skeleton(), animations()
    out = {"what": "the reference's evalIK (animation/controller.cpp:166-265), sliced, one thread, on the poses the two SAMPLE layers leave; scaled from `sample` instances",
           "instances": args.instances, "sample": args.sample, "reps": args.reps}
    for mode in ("b", "c"):
        ins = programs(args.sample, mode, [0, 1])
        jobs = []
        for i in range(args.sample):
            p, r = oracle.update_animators(anims, [[(int(x["animation"]), float(x["weight"]), int(x["time"]), bool(x["looped"])) for x in ins[i, :2]]], s["bind"])
            for x in ins[i, 2:]:
                jobs.append((s["parents"], float(x["alpha"]), x["target"], int(x["leaf_bone"]), int(x["bones_count"]), p[0], r[0]))
        job = os.path.join(d, f"{mode}.bin")
        open(job, "wb").write(R.job_bytes(jobs))
        runs = []
        for _ in range(5):
            n_jobs, reps, ms = subprocess.run([exe, job, os.path.join(d, "out.bin"), "time", str(args.reps)], check=True, capture_output=True, text=True).stdout.split()
            runs.append(float(ms) / int(reps) / args.sample * args.instances)
        out[mode] = {"ik_per_instance": len(CHAINS[mode]), "ms_for_all_instances_median": float(np.median(runs)), "min": float(np.min(runs)), "max": float(np.max(runs)),
                     "us_per_instance": float(np.median(runs)) * 1e3 / args.instances}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if args.reference:
        return reference(args)
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
    K_ANIM = api.KERNEL_NAMES.index("anim_update")
    work = {}
    for mode in ("a_old", "a_new", "b", "c"):
        ins = programs(n, mode, ids)
        first = (np.arange(n + 1, dtype=np.uint32) * ins.shape[1]).astype(np.uint32)
        if mode == "a_old":
            rec = np.zeros(ins.shape, api.BLEND_SAMPLE)
            for f in ("animation", "weight", "time", "looped"):
                rec[f] = ins[f]
            work[mode] = (sk.lib.lmx_anim_eval_blend_stacks, first, np.ascontiguousarray(rec.reshape(-1)))
        else:
            work[mode] = (sk.lib.lmx_anim_eval_blend_instrs, first, np.ascontiguousarray(ins.reshape(-1)))
    ctx.profile_enable(True)

    def call(mode):
        fn, first, rec = work[mode]
        ctx.profile_reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        ctx.check(fn(ctx.h, n, api._ptr(first), api._ptr(rec)))
        b.record()
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ms, launches = ctx.profile_get(K_ANIM)
        assert launches == 1, launches
        return ms * 1e3, a.elapsed_time(b) * 1e3, wall * 1e3

    rows = {m: [] for m in work}
    for m in work:  # warm-up of every shape
        for _ in range(3):
            call(m)
    poses = {}
    for r in range(args.rounds):
        for m in work:
            rows[m].append([call(m) for _ in range(args.steps)])
            if r == 0 and m in ("a_old", "a_new"):
                poses[m] = [sk.readRelativePose(i) for i in (0, n // 2, n - 1)]
    same = all(np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(poses["a_old"], poses["a_new"]))
    out = {"instances": n, "bones": BONES, "steps": args.steps, "rounds": args.rounds, "a_new_equals_a_old_bitwise": bool(same), "modes": {}}
    for m, rounds in rows.items():
        t = np.array(rounds)  # [round, step, (kernel, span, wall)]
        out["modes"][m] = {name: {"median_us": float(np.median(t[:, :, k])), "min_us": float(t[:, :, k].min()), "max_us": float(t[:, :, k].max()),
                                  "round_medians_us": [float(np.median(t[r, :, k])) for r in range(t.shape[0])]}
                           for k, name in enumerate(("kernel", "stream_span", "host_wall"))}
    ctx.close()
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
