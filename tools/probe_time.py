#!/usr/bin/env python
"""Times the probe bake on the device (lmx_probes_*) at the reference's capture size, 128:
  environment probes  batches of 1, 16 and 256: set_cubemaps (the host's finite check and the upload), sh_run, read_sh;
  reflection probes   batches of 1 and 16: set_cubemaps, filter_run (mip chain, five radiance levels, RGBM), read_rgbm.
--rounds rounds of --steps runs each; per step the wall time of each call up to the synchronise behind it (the first sh_run of a size,
which also builds that size's table, is the warm-up round's). One JSON line with the medians, and profiles/probes/README.md (--out) with
the same numbers as a table next to the reference's one-thread time of SphericalHarmonics::compute, where --reference-ms gives it
(tests/test_probe_oracle_vs_ref.py prints that figure where the reference tree exists). No bar is fixed.

    python tools/probe_time.py [--steps 5] [--rounds 3] [--out profiles/probes/README.md] [--reference-ms 35.7]
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
from tests import probe_oracle as PO  # noqa: E402  (the log-uniform colours of the tests)

SIZE = 128


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def batch(n):
    one = PO.hdr_cubemaps(7, min(n, 4), SIZE)
    return np.ascontiguousarray(np.tile(one, ((n + len(one) - 1) // len(one), 1, 1, 1, 1))[:n])


def shape(ctx, kind, n, steps, rounds):
    pb = api.ProbeBaker(ctx)
    cm = batch(n)
    calls = {"set_cubemaps": lambda: pb.setCubemaps(cm)}
    if kind == "environment":
        calls["run"] = pb.shRun
        calls["read"] = pb.readSH
    else:
        calls["run"] = pb.filterRun
        calls["read"] = lambda: pb.lib.lmx_probes_read_rgbm(pb.h, out.ctypes.data, out.size)
        out = np.zeros(n * 4 * sum(6 * (SIZE >> k) ** 2 for k in range(api.PROBE_LEVELS)), np.uint8)
    per = {k: [] for k in calls}
    for r in range(rounds + 1):  # (round 0 warms up)
        one = {k: [] for k in calls}
        for _ in range(steps):
            for k, call in calls.items():
                one[k].append(timed(ctx, call))
        if r:
            for k in per:
                per[k].append(float(np.median(one[k])))
    pb.close()
    res = {"kind": kind, "probes": n, "size": SIZE, "megabytes": cm.nbytes / 1e6}
    for k, ms in per.items():
        res[k + "_ms"] = float(np.median(ms))
        res[k + "_round_medians_ms"] = ms
    return res


def readme(rows, args):
    lines = ["# Probe bake on the device: timings", "",
             "Written by `tools/probe_time.py` (DESIGN.md §4.22). Cubemaps of %d, log-uniform colours; medians over %d rounds of %d runs, wall time of each" % (SIZE, args.rounds, args.steps),
             "call up to the synchronise behind it. `set_cubemaps` is the host's finite check and the upload of the batch; `run` is `sh_run` for",
             "environment probes (table of the size already built) and `filter_run` (mip chain, five radiance levels, RGBM) for reflection probes;",
             "`read` is `read_sh` / `read_rgbm`.", "",
             "| probes | kind | batch MB | set_cubemaps ms | run ms | run ms per probe | read ms |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %s | %.1f | %.3f | %.3f | %.3f | %.3f |" % (r["probes"], r["kind"], r["megabytes"], r["set_cubemaps_ms"], r["run_ms"], r["run_ms"] / r["probes"], r["read_ms"]))
    lines.append("")
    if args.reference_ms is not None:
        lines.append("The reference's `SphericalHarmonics::compute` on one 6 x 128 x 128 capture (the editor's size), one thread of the development machine's CPU: %.1f ms" % args.reference_ms)
        lines.append("(tests/test_probe_oracle_vs_ref.py prints it). It is the CPU side of the comparison for an environment probe, not a bar.")
    else:
        lines.append("The reference's one-thread time of `SphericalHarmonics::compute`: not measured in this run.")
    lines += ["", "Not measured: the radiance filter has no CPU counterpart in the reference (it is a pixel shader there), so `filter_run` stands alone;",
              "the kernels' own time apart from the host's share of each call; other capture sizes; the engine's capture, compression and file writes.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probes", "README.md"))
    ap.add_argument("--reference-ms", type=float, default=None)
    ap.add_argument("--size", type=int, default=128, help="the cubemaps' size (a power of two of 16 or more); the table's text assumes 128")
    a = ap.parse_args()
    SIZE = a.size
    ctx = api.Context(0)
    rows = [shape(ctx, "environment", n, a.steps, a.rounds) for n in (1, 16, 256)] + [shape(ctx, "reflection", n, a.steps, a.rounds) for n in (1, 16)]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(readme(rows, a))
    print(json.dumps({"tool": "probe_time", "steps": a.steps, "rounds": a.rounds, "shapes": rows}))
