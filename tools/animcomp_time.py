#!/usr/bin/env python
"""Times the animation compressor on the device (lmx_animcomp_set_clips / lmx_animcomp_run): one importer-sized batch -
32 clips of 60 bones and 300 samples - and one single clip of the same shape. The keys are unit rotations around a per-bone axis and
positions on smooth curves; a quarter of the bones stay at the bind position. --rounds rounds of --steps runs each; per step the wall time of
lmx_animcomp_run up to the synchronise behind it (it holds the run's one host wait), and of the Python binding's setClips with the buffers
already allocated (the key upload). Next to them: the algorithmic bytes - every key read twice, the ranges' pass and the pack's, plus the
streams written - and the share of the HBM rate (--hbm-gbs, 8000 by default: the card's nominal rate) they imply at the measured time; and
the time of the same clips through lmx_animcomp_compress_host, the library's own arithmetic on one CPU thread. The reference's own loop on
one clip of this shape is timed by tests/test_animcomp_oracle_vs_ref.py where the reference tree exists (it prints it); --reference-ms and
--reference-cpu hand that figure and the CPU it was measured on to the table. One JSON line with the medians, and
profiles/animcomp/README.md (--out) with the same numbers as a table. No bar is fixed.

    python tools/animcomp_time.py [--steps 5] [--rounds 3] [--out profiles/animcomp/README.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumixengine_amd import api  # noqa: E402


def make_clip(rng, n_bones, n_samples):
    t = np.linspace(0.0, 1.0, n_samples, dtype=np.float64)[:, None]
    keys = np.zeros((n_samples, n_bones), api.ANIM_KEY)
    bind = rng.uniform(-1, 1, (n_bones, 3)).astype(np.float32)
    swing = rng.uniform(0.0, 0.3, (1, n_bones, 3)) * (rng.random((1, n_bones, 1)) > 0.25)
    keys["pos"] = (bind[None] + swing * np.sin(2 * np.pi * (t[:, :, None] * rng.uniform(0.5, 3, (1, n_bones, 3))))).astype(np.float32)
    axis = rng.normal(size=(n_bones, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0.1, 1.5, (1, n_bones)) * np.sin(2 * np.pi * t * rng.uniform(0.5, 2, (1, n_bones))) + rng.uniform(-1, 1, (1, n_bones))
    keys["rot"][:, :, :3] = (axis[None] * np.sin(angle / 2)[:, :, None]).astype(np.float32)
    keys["rot"][:, :, 3] = np.cos(angle / 2).astype(np.float32)
    return dict(keys=keys, bind=bind, has_keys=None, fps=30.0, translation_error=1.0, rotation_error=1.0)


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shape(ctx, name, n_clips, n_bones, n_samples, a):
    rng = np.random.default_rng(7)
    clips = [make_clip(rng, n_bones, n_samples) for _ in range(n_clips)]
    ac = api.AnimCompressor(ctx)
    ac.setClips(clips)  # (the first set and run of a shape allocate the device buffers: not timed)
    ac.run()
    res = {"shape": name, "clips": n_clips, "bones": n_bones, "samples": n_samples}
    res["set_clips_ms"] = float(np.median([timed(ctx, lambda: ac.setClips(clips)) for _ in range(a.steps)]))
    per = []
    for r in range(a.rounds + 1):  # (round 0 warms up)
        one = [timed(ctx, ac.run) for _ in range(a.steps)]
        if r:
            per.append(float(np.median(one)))
    res["run_ms"], res["run_round_medians_ms"] = float(np.median(per)), per
    infos = [ac.clipInfo(i) for i in range(n_clips)]
    assert all(i["status"] == 0 for i in infos)
    key_bytes = 28 * n_clips * n_bones * n_samples
    stream_bytes = sum(i["translation_stream_size"] + i["rotation_stream_size"] for i in infos)
    res.update(key_megabytes=key_bytes / 1e6, stream_megabytes=stream_bytes / 1e6, algorithmic_megabytes=(2 * key_bytes + stream_bytes) / 1e6)
    res["hbm_share"] = (2 * key_bytes + stream_bytes) / (res["run_ms"] * 1e-3) / (a.hbm_gbs * 1e9)
    res["mean_frame_bits"] = [float(np.mean([i["translations_frame_size_bits"] for i in infos])), float(np.mean([i["rotations_frame_size_bits"] for i in infos]))]
    ac.close()
    t0 = time.perf_counter()
    for c in clips[: a.host_clips]:
        api.animcomp_compress_host(c)
    res["host_one_thread_ms"] = (time.perf_counter() - t0) * 1e3 / min(a.host_clips, n_clips) * n_clips  # (scaled from the clips timed)
    return res


def readme(rows, a):
    lines = ["# Animation compressor on the device: timings", "",
             "Written by `tools/animcomp_time.py` (DESIGN.md §4.25). Medians over %d rounds of %d runs; `run` is the wall time of `lmx_animcomp_run` up to the" % (a.rounds, a.steps),
             "synchronise behind it - three launches, and between the second and the third the run's one host wait, the read of the clips' infos.",
             "`set` is the Python binding's `setClips` with the buffers already allocated: the transposition to records on the host and the key upload.",
             "Algorithmic bytes: every key twice (the range fold, the pack) and the streams once; the share is what they imply of %.0f GB/s at the" % a.hbm_gbs,
             "measured time. `host` is the same clips through `lmx_animcomp_compress_host`, the library's arithmetic on one CPU thread, called from Python",
             "(two calls per clip: the info, then the arrays).", "",
             "| shape | clips | bones | samples | keys MB | streams MB | set ms | run ms | algorithmic MB | share of HBM rate | host, one thread ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %d | %d | %.2f | %.2f | %.3f | %.3f | %.2f | %.2f %% | %.1f |" % (
            r["shape"], r["clips"], r["bones"], r["samples"], r["key_megabytes"], r["stream_megabytes"], r["set_clips_ms"], r["run_ms"], r["algorithmic_megabytes"], 100 * r["hbm_share"],
            r["host_one_thread_ms"]))
    lines.append("")
    if a.reference_ms is not None and a.reference_cpu:
        lines.append("The reference's own loop on one thread of a %s (tests/test_animcomp_oracle_vs_ref.py prints it): %.2f ms for one clip of 60 bones and" % (a.reference_cpu, a.reference_ms))
        lines.append("300 samples, other keys of the same kind. It is the CPU side of the comparison, not a bar.")
    else:
        lines.append("The reference's own loop on one CPU thread: not measured in this run.")
    lines += ["", "Not measured: the kernels' own times apart from the host's share of a call (launches, the read of the infos, the synchronise); which of the",
              "three kernels takes the most; occupancy; clips that are not smooth curves; the importer's fillTracks in front and the file write behind.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "animcomp", "README.md"))
    ap.add_argument("--json", default=None, help="also write the JSON line to this file")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--host-clips", type=int, default=4, help="clips timed through the host entry")
    ap.add_argument("--reference-ms", type=float, default=None, help="the reference's loop on one clip of 60 bones x 300 samples")
    ap.add_argument("--reference-cpu", default=None, help="the CPU --reference-ms was measured on")
    ap.add_argument("--quick", action="store_true", help="small shapes only (a check that the tool runs)")
    a = ap.parse_args()
    shapes = [("importer batch", 32, 60, 300), ("single clip", 1, 60, 300)]
    if a.quick:
        shapes = [("quick batch", 3, 8, 40), ("quick clip", 1, 8, 40)]
    ctx = api.Context(0)
    rows = [shape(ctx, *s, a) for s in shapes]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(readme(rows, a))
    line = json.dumps({"tool": "animcomp_time", "steps": a.steps, "rounds": a.rounds, "hbm_gbs": a.hbm_gbs, "shapes": rows})
    if a.json:
        open(a.json, "w").write(line + "\n")
    print(line)
