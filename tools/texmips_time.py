#!/usr/bin/env python
"""Times the mip chains on the device (lmx_texcomp_set_chains / generate_mips): one 1024 x 1024 chain, one 4096 x 4096
chain, six faces of 4096 x 4096, and a batch of 256 chains of 37 x 21; each in the linear, the sRGB and the stochastic mode without coverage
scaling, and in the sRGB mode with it. The pixels are uniform noise. --rounds rounds of --steps runs each; per step the wall time of
lmx_texcomp_generate_mips up to the synchronise behind it, and next to it lmx_texcomp_run(BC1)'s time for the same chains (one round; the
six 4096 x 4096 faces are left out of it with --no-big-run). One JSON line with the medians, and profiles/texmips/README.md (--out) with
the same numbers as a table next to the reference's one-thread times per output texel where --reference-ns gives them
together with --reference-cpu, the name of the CPU they were measured on (tests/test_texmips_oracle_vs_ref.py prints them where the
reference tree exists). No bar is fixed.

    python tools/texmips_time.py [--steps 3] [--rounds 2] [--out profiles/texmips/README.md] [--reference-ns 44.5 57.2]
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

MODES = (("linear", api.TEXMIP_LINEAR, -1.0), ("srgb", api.TEXMIP_SRGB, -1.0), ("stochastic", api.TEXMIP_STOCHASTIC, -1.0), ("srgb_coverage", api.TEXMIP_SRGB, 0.5))


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shape(ctx, name, n, w, h, steps, rounds, with_run):
    rng = np.random.default_rng(1)
    tile = rng.integers(0, 256, (1 << 22, 4), dtype=np.uint8)
    images = np.resize(tile, (n * h * w, 4)).reshape(n, h, w, 4)  # (the noise repeats every 4 M pixels)
    levels = api.texcomp_chain_levels(w, h)
    tc = api.TexCompressor(ctx)
    first_small = next(m for m in range(levels) if max(w >> m, 1) <= 32 and max(h >> m, 1) <= 32)  # the levels behind it are one k_mip_tail
    tail = 1 if first_small + 1 < levels else 0
    res = {"shape": name, "chains": n, "levels": levels, "megapixels_level0": n * w * h / 1e6, "launches_plain": first_small + tail, "launches_coverage": 2 * first_small + tail + 1}
    tc.setChains(images)  # (the first set of a shape allocates the device buffers: not timed)
    res["set_chains_ms"] = float(np.median([timed(ctx, lambda: tc.setChains(images)) for _ in range(steps)]))
    for mname, mode, ref_norm in MODES:
        per = []
        for r in range(rounds + 1):  # (round 0 warms up)
            one = [timed(ctx, lambda: tc.generateMips(mode, ref_norm)) for _ in range(steps)]
            if r:
                per.append(float(np.median(one)))
        res[mname + "_ms"] = float(np.median(per))
        res[mname + "_round_medians_ms"] = per
    if with_run:
        tc.run(api.TEX_BC1)  # (warms up)
        res["BC1_run_ms"] = float(np.median([timed(ctx, lambda: tc.run(api.TEX_BC1)) for _ in range(steps)]))
    tc.close()
    return res


def readme(rows, args):
    lines = ["# Mip chains on the device: timings", "",
             "Written by `tools/texmips_time.py` (DESIGN.md §4.24). Uniform noise; medians over %d rounds of %d runs, wall time of" % (args.rounds, args.steps),
             "`lmx_texcomp_generate_mips` up to the synchronise behind it (the host's share of the launches included). `set` is the Python binding's",
             "`setChains` with the buffers already allocated; `BC1` is `lmx_texcomp_run(LMX_TEX_BC1)` on the same chains, %d runs. Launches per chain" % args.steps,
             "batch: one per level down to the first of at most 32 x 32 and one k_mip_tail for the levels behind it; with coverage scaling one more per",
             "level launch, the count over image 0 and a fill.", "",
             "| shape | chains | levels | Mpixel of level 0 | launches (with coverage) | set ms | linear ms | sRGB ms | stochastic ms | sRGB + coverage ms | BC1 run ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %d | %.2f | %d (%d + fill) | %.2f | %.3f | %.3f | %.3f | %.3f | %s |" % (
            r["shape"], r["chains"], r["levels"], r["megapixels_level0"], r["launches_plain"], r["launches_coverage"], r["set_chains_ms"], r["linear_ms"], r["srgb_ms"], r["stochastic_ms"],
            r["srgb_coverage_ms"], "%.2f" % r["BC1_run_ms"] if "BC1_run_ms" in r else "not run"))
    lines.append("")
    if args.reference_ns is not None and args.reference_cpu:
        lines.append("The reference's `stbir_resize_uint8_linear` / `_srgb` on one thread of a %s, per output texel" % args.reference_cpu)
        lines.append("(tests/test_texmips_oracle_vs_ref.py prints it, on images of at most 64 x 64): %.1f ns / %.1f ns. It is the CPU side of the comparison, not a bar." % tuple(args.reference_ns))
    else:
        lines.append("The reference's one-thread times per output texel: not measured in this run.")
    lines += ["", "Not measured: the kernels' own time apart from the host's share of a call (launch, synchronise); occupancy and what bounds k_mip_level;",
              "images that are not noise; the image decode in front of the chains and the file write behind the blocks.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texmips", "README.md"))
    ap.add_argument("--json", default=None, help="also write the JSON line to this file")
    ap.add_argument("--reference-ns", type=float, nargs=2, default=None, metavar=("LINEAR", "SRGB"))
    ap.add_argument("--reference-cpu", default=None, help="the CPU --reference-ns was measured on")
    ap.add_argument("--no-big-run", action="store_true", help="leave lmx_texcomp_run out for the six 4096 x 4096 faces")
    ap.add_argument("--quick", action="store_true", help="small shapes only (a check that the tool runs)")
    a = ap.parse_args()
    shapes = [("1024 x 1024", 1, 1024, 1024, True), ("4096 x 4096", 1, 4096, 4096, True), ("4096 x 4096 x 6 faces", 6, 4096, 4096, not a.no_big_run), ("37 x 21 x 256", 256, 37, 21, True)]
    if a.quick:
        shapes = [("64 x 64", 1, 64, 64, True), ("37 x 21 x 7", 7, 37, 21, True)]
    ctx = api.Context(0)
    rows = [shape(ctx, name, n, w, h, a.steps, a.rounds, with_run) for name, n, w, h, with_run in shapes]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(readme(rows, a))
    line = json.dumps({"tool": "texmips_time", "steps": a.steps, "rounds": a.rounds, "shapes": rows})
    if a.json:
        open(a.json, "w").write(line + "\n")
    print(line)
