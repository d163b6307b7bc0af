#!/usr/bin/env python
"""Times structural edits of the world mirror on BASELINE config 3's hierarchy (--roots x chains of depth 4: 1 M entities by default),
every entity bound to the culling system and the moved list tracked:
  edit_one_reparent   lmx_world_edit with one re-parenting
  edit_3k             lmx_world_edit with 1 k destroys + 1 k creates + 1 k re-parentings
  set_parent          the unchanged lmx_world_set_parent (one re-parenting: both transform sets down, a host BFS, both sets up again)
all as host wall time up to the synchronise, on one world in one process. A round is --steps calls of each of the three, one after the
other (lmx_world_set_parent rebuilds the mirror from the host, so the edit that follows it states `parent` on the device again: the
first edit of a round pays that upload and is reported on its own, not in the medians). One JSON line: medians per round. Nothing is
asserted: `holds` states DESIGN.md 4.4.1's comparison for this run.

    python tools/world_edit_time.py [--roots 250000] [--steps 5] [--rounds 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.zeros(1, device="cuda")  # torch opens the device before the library does
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = scenes.hierarchy_chains(args.roots, 4, seed=2)
    parent = h["parent"].copy()
    n = len(parent)
    roots = np.flatnonzero(parent < 0).astype(np.int32)
    tr = h["local"].copy()
    w = api.World(ctx)
    w.trackMoved(True)
    w.build(parent, tr)
    w.propagate()
    world0 = w.getTransforms()
    rng = np.random.default_rng(5)
    ent = np.arange(n, dtype=np.int32)
    radius = rng.uniform(0.5, 40.0, n).astype(np.float32)
    cs = api.CullingSystem(ctx)
    cs.build(ent, np.zeros(n, np.uint8), world0["pos"], radius)
    w.bindCulling(ent, radius)
    w.propagate()  # states the binding tables on the device
    w.readMoved()
    has_child = np.zeros(n, bool)
    has_child[parent[parent >= 0]] = True
    leaves = np.flatnonzero(~has_child & (parent >= 0)).astype(np.int32)
    k = min(1000, len(leaves) // 4)
    groups = [leaves[:k], leaves[k : 2 * k]]  # destroyed and created again in turns
    movers = leaves[2 * k : 3 * k]
    one = int(leaves[3 * k])
    create_tr = scenes.random_transforms(rng, k, 900.0)
    state = {"step": 0}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def edit_one():
        return timed(lambda: w.edit(reparent=[(int(rng.choice(roots)), one)]))

    def edit_3k():
        s = state["step"]
        state["step"] += 1
        destroy = groups[s % 2]
        create = groups[(s + 1) % 2] if s else np.arange(n, n + k, dtype=np.int32)  # (the first step grows the range instead)
        rp = np.stack([rng.choice(roots, size=k), movers], axis=1)
        return timed(lambda: w.edit(destroy=destroy, create=create, create_transforms=create_tr, reparent=rp))

    def set_parent():
        return timed(lambda: w.setParent(int(rng.choice(roots)), one))

    edit_one(), edit_3k(), set_parent()  # warm-up of the three
    w.propagate()
    out_rounds = {"edit_one_reparent": [], "edit_3k": [], "set_parent": []}
    first_after_rebuild = []
    for r in range(args.rounds):
        first_after_rebuild.append(edit_one())
        for name, fn in (("edit_one_reparent", edit_one), ("edit_3k", edit_3k), ("set_parent", set_parent)):
            out_rounds[name].append([fn() for _ in range(args.steps)])
        w.propagate()  # (the binding tables again after the rebuilds, outside the timing)
        w.readMoved()
    info = w.info()

    def stats(t):
        t = np.array(t)
        return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()), "round_medians_us": [float(np.median(x)) for x in t]}

    out = {"entities": n, "roots": int(args.roots), "steps": args.steps, "rounds": args.rounds, "info_at_end": info, "first_edit_after_a_rebuild_us": first_after_rebuild}
    out.update({name: stats(t) for name, t in out_rounds.items()})
    old = out["set_parent"]["round_medians_us"]
    spread = max(old) - min(old)
    out["holds"] = {name: bool(max(out[name]["round_medians_us"]) < min(old) - spread) for name in ("edit_one_reparent", "edit_3k")}
    out["holds"]["spread_of_set_parent_round_medians_us"] = spread
    ctx.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
