#!/usr/bin/env python
"""Times the texture compressor on the device (lmx_texcomp_*):
  probes   1, 16 and 256 reflection probes' worth of RGBM images at the reference's capture size, 128: per probe six faces of levels
           128 .. 8, 30 images (what saveCubemap hands TextureCompressor::compress);
  images   one 1024 x 1024 and one 4096 x 4096 image;
each in BC1, BC3 and BC5. The pixels are uniform noise: no block is solid and no search ends early. --rounds rounds of --steps runs each;
per step the wall time of lmx_texcomp_run up to the synchronise behind it; per shape the median of --steps set_images (the binding's
concatenation of the images and the upload; the first set of a shape, which allocates, is not timed) and one read-back. One JSON line with the medians, and profiles/texcomp/README.md (--out) with the same numbers as a
table next to the reference's one-thread times per block, where --reference-us gives them (tests/test_texcomp_oracle_vs_ref.py prints
them where the reference tree exists). No bar is fixed.

    python tools/texcomp_time.py [--steps 3] [--rounds 2] [--out profiles/texcomp/README.md] [--reference-us 4.9 120.9]
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

FORMATS = (("BC1", api.TEX_BC1), ("BC3", api.TEX_BC3), ("BC5", api.TEX_BC5))


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shape(ctx, name, sizes, steps, rounds):
    rng = np.random.default_rng(1)
    tile = rng.integers(0, 256, (1 << 22, 4), dtype=np.uint8)
    images = [np.resize(tile, (h * w, 4)).reshape(h, w, 4) for w, h in sizes]  # (the noise repeats every 4 M pixels)
    tc = api.TexCompressor(ctx)
    res = {"shape": name, "images": len(images), "megapixels": sum(w * h for w, h in sizes) / 1e6, "blocks": int(sum(((w + 3) >> 2) * ((h + 3) >> 2) for w, h in sizes))}
    tc.setImages(images)  # (the first set of a shape allocates the device buffers: not timed)
    res["set_images_ms"] = float(np.median([timed(ctx, lambda: tc.setImages(images)) for _ in range(steps)]))
    for fname, fmt in FORMATS:
        per = []
        for r in range(rounds + 1):  # (round 0 warms up)
            one = [timed(ctx, lambda: tc.run(fmt)) for _ in range(steps)]
            if r:
                per.append(float(np.median(one)))
        res[fname + "_run_ms"] = float(np.median(per))
        res[fname + "_round_medians_ms"] = per
        res[fname + "_read_ms"] = timed(ctx, tc.read)
    tc.close()
    return res


def readme(rows, args):
    lines = ["# Texture compressor on the device: timings", "",
             "Written by `tools/texcomp_time.py` (DESIGN.md §4.23). Uniform noise (no solid block, no search that ends early); medians over %d rounds of %d runs," % (args.rounds, args.steps),
             "wall time of `lmx_texcomp_run` up to the synchronise behind it. `set` is the Python binding's `setImages`: the concatenation of the images",
             "and `lmx_texcomp_set_images`' upload, buffers already allocated. A probe is six faces of levels 128 .. 8 of RGBM, 30 images.", "",
             "| shape | images | Mpixel | blocks | set ms | BC1 ms | BC3 ms | BC5 ms | BC1 ns per block | BC3 ns per block |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %.2f | %d | %.2f | %.3f | %.3f | %.3f | %.1f | %.1f |" % (r["shape"], r["images"], r["megapixels"], r["blocks"], r["set_images_ms"], r["BC1_run_ms"],
                                                                                    r["BC3_run_ms"], r["BC5_run_ms"], r["BC1_run_ms"] * 1e6 / r["blocks"], r["BC3_run_ms"] * 1e6 / r["blocks"]))
    lines.append("")
    if args.reference_us is not None:
        lines.append("The reference's `rgbcx::encode_bc1` on the development machine's CPU, one thread, per block (tests/test_texcomp_oracle_vs_ref.py prints it):")
        lines.append("level 10 (what the engine calls) %.2f us, the exhaustive mode (what the device computes) %.1f us. It is the CPU side of the comparison, not a bar." % tuple(args.reference_us))
    else:
        lines.append("The reference's one-thread times per block: not measured in this run.")
    lines += ["", "Not measured: the kernels' own time apart from the host's share of a call (launch, synchronise); occupancy and what bounds k_bc1_search;",
              "images that are not noise (solid blocks take a shortcut, blocks whose first endpoints are exact skip the search); the engine's mip",
              "generation and file writes.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texcomp", "README.md"))
    ap.add_argument("--json", default=None, help="also write the JSON line to this file")
    ap.add_argument("--reference-us", type=float, nargs=2, default=None, metavar=("LEVEL10", "EXHAUSTIVE"))
    ap.add_argument("--quick", action="store_true", help="small shapes only (a check that the tool runs)")
    a = ap.parse_args()
    probe = [(128 >> k, 128 >> k) for _ in range(6) for k in range(api.PROBE_LEVELS)]
    shapes = [("1 probe", probe), ("16 probes", probe * 16), ("256 probes", probe * 256), ("1024 x 1024", [(1024, 1024)]), ("4096 x 4096", [(4096, 4096)])]
    if a.quick:
        shapes = [("1 probe of 16", [(16 >> k, 16 >> k) for _ in range(6) for k in range(api.PROBE_LEVELS)]), ("64 x 64", [(64, 64)])]
    ctx = api.Context(0)
    rows = [shape(ctx, name, sizes, a.steps, a.rounds) for name, sizes in shapes]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(readme(rows, a))
    line = json.dumps({"tool": "texcomp_time", "steps": a.steps, "rounds": a.rounds, "shapes": rows})
    if a.json:
        open(a.json, "w").write(line + "\n")
    print(line)
