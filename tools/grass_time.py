#!/usr/bin/env python
"""Times terrain grass on the device (lmx_grass_*): 4 terrains x 4 grass types, distance 100, spacing 0.5 - 13 x 13 = 169 quads
per type, 2704 in all - over 2048 x 2048 maps.
  cut    a frame where every quad is new (the terrains invalidated before it),
  walk   a frame whose centre has moved one quad along x: one row of 13 quads per type is new,
  cull   every cached quad against five views (main plus four orthographic cascades).
--rounds rounds of --steps frames each; per frame the host's time in the call (it returns with the launch enqueued) and the wall time up to the
synchronise behind it. One JSON line: medians per frame kind and per round, the accepted samples and the algorithmic bytes of the cut frame
(64 B written per accepted sample; read: the splat window of every quad at 4 B a texel, three heightmap texels of 2 B per accepted sample).

    python tools/grass_time.py [--steps 10] [--rounds 3]
    python tools/grass_time.py --reference      # one-thread CPU time of the reference's createGrass / quad loop (needs the reference tree, no GPU)

--reference cuts createGrass and renderGrass's quad loop out of the reference tree as tests/test_grass_oracle_vs_ref.py does, runs the same
three frames per terrain in one thread, sums the harness' own clock readings over the four terrains and writes profiles/grass/reference_cpu.json.
No bar is fixed.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumixengine_amd import api  # noqa: E402

TERRAINS, TYPES, MAP, DISTANCE, SPACING = 4, 4, 2048, 100.0, 0.5
CENTRE = (1000.0, 1000.0)
QUAD = SPACING * 32


def terrains():
    out = []
    for k in range(TERRAINS):
        rng = np.random.default_rng(100 + k)
        hm = rng.integers(0, 65536, (MAP, MAP)).astype(np.uint16)
        on = rng.random((MAP, MAP)) < 0.5
        splat = (np.where(on, rng.integers(1, 16, (MAP, MAP)), 0).astype(np.uint32) << np.uint32(16)).astype(np.uint32)
        types = [(SPACING, DISTANCE, api.GRASS_ROTATION_Y_UP if t % 2 == 0 else api.GRASS_ROTATION_ALL_RANDOM, 1) for t in range(TYPES)]
        out.append({"key": f"time{k}", "entity": k, "heightmap": hm, "splatmap": splat, "scale": np.float32([1.0, 40.0, 1.0]), "types": types})
    return out


def positions():
    return np.array([[k * 3000.0, 0.0, 0.0] for k in range(TERRAINS)])


def views(pos):
    cam = pos[0] + (CENTRE[0], 20.0, CENTRE[1])
    v = np.zeros(5, api.GRASS_VIEW)
    v["viewport_pos"], v["lod_multiplier"] = cam, 1.0
    v["frustum"][0] = api.frustum_perspective(cam, (-0.6, 0.3, -0.74), (0, 1, 0), 1.0, 1.6, 0.1, 400.0)[0]
    for k, size in enumerate((20.0, 45.0, 90.0, 200.0)):
        v["frustum"][1 + k] = api.frustum_ortho(cam + (5.0, 80.0, 5.0), (-0.3, 0.9, -0.2), (0, 0, 1), size, size, 0.0, 300.0)[0]
    return v


def timed(ctx, call):
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    ctx.synchronize()
    return (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6


def device(args):
    ctx = api.Context(0)
    ts, pos = terrains(), positions()
    g = api.Grass(ctx)
    g.reserve(2 * TERRAINS * TYPES * 169)
    g.setTerrains(ts)
    g.setPositions(pos)
    vs = views(pos)
    centres = np.tile(np.float32(CENTRE), (TERRAINS, 1))
    rounds = {"cut": [], "walk": [], "cull": []}
    frame = 10
    accepted = window_texels = 0
    for r in range(args.rounds + 1):  # (round 0 warms up)
        per = {"cut": [], "walk": [], "cull": []}
        for s in range(args.steps):
            g.invalidate()
            ctx.synchronize()
            frame += 10
            per["cut"].append(timed(ctx, lambda: g.update(frame, centres)))
            if r == 0 and s == 0:
                q = g.readQuads()
                accepted = int(q["instances_count"].sum()) // 2
                window_texels = len(q) * (int(QUAD) + 1) ** 2
                assert len(q) == TERRAINS * TYPES * 169, len(q)
            moved = centres + np.float32([QUAD, 0.0])
            per["walk"].append(timed(ctx, lambda: g.update(frame + 1, moved)))
            per["cull"].append(timed(ctx, lambda: g.cull(vs)))
        if r:
            for k in rounds:
                rounds[k].append([float(np.median([p[0] for p in per[k]])), float(np.median([p[1] for p in per[k]]))])
    out = {"tool": "grass_time", "terrains": TERRAINS, "types": TYPES, "quads_cut_frame": TERRAINS * TYPES * 169, "quads_walk_frame": TERRAINS * TYPES * 13,
           "accepted_samples_cut_frame": accepted, "steps": args.steps, "rounds": args.rounds,
           "cut_frame_bytes": {"written": 64 * accepted, "window_read": 4 * window_texels, "height_read": 6 * accepted}}
    for k, v in rounds.items():
        out[k] = {"call_us_median": float(np.median([x[0] for x in v])), "to_sync_us_median": float(np.median([x[1] for x in v])), "round_medians_us": v}
    counts = g.counts()
    out["cull_counts"] = [[int(c["draws"]), int(c["culled"]), int(c["instances"])] for c in counts]
    print(json.dumps(out))
    g.close()
    ctx.close()


def reference(args):
    from tests import test_grass_oracle_vs_ref as T

    ts, pos = terrains(), positions()
    vs = views(pos)
    total = {"cut": 0, "walk": 0, "cull": 0}
    with tempfile.TemporaryDirectory(prefix="lmx_grass_time_") as d:
        ref = (T.build_harness(d), d)
        for k, t in enumerate(ts):
            times = {}
            T.run_ref(ref, t, [(20, CENTRE, False), (21, (CENTRE[0] + QUAD, CENTRE[1]), False)], pos[k], vs, times)
            total["cut"] += times["frame"][0]
            total["walk"] += times["frame"][1]
            total["cull"] += sum(times["view"])
    out = {"tool": "grass_time --reference", "threads": 1, "terrains": TERRAINS, "types": TYPES, "quads_cut_frame": TERRAINS * TYPES * 169,
           "cut_ms": total["cut"] / 1e6, "walk_ms": total["walk"] / 1e6, "cull_five_views_one_mesh_ms": total["cull"] / 1e6}
    os.makedirs(os.path.join(ROOT, "profiles", "grass"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "grass", "reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    reference(a) if a.reference else device(a)
