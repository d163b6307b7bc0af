#!/usr/bin/env python
"""Writes tests/golden/ribbons_small.npz: what the reference's own ribbon code - cut out of its tree and compiled behind the shim of
tests/test_ribbon_oracle_vs_ref.py - gives for the scripts tests/ribbon_cases.GOLDEN, after every op: per emitter the particle count, the
ribbon records, the live points of every channel and the slice rows (packed per ribbon: the gather of the rows the reference's output
program gives for every physical slot, DESIGN §4.15.1 deviation a). Data only; needs the reference tree and no GPU.

    python tests/golden/make_golden_ribbons.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import ribbon_cases as C  # noqa: E402
from tests import test_ribbon_oracle_vs_ref as T  # noqa: E402


def main():
    d = tempfile.mkdtemp(prefix="ribbons_golden_")
    exe = T.build_harness(d)
    out = {}
    for case in C.GOLDEN:
        systems, options, _, ops = C.CASES[case]
        for k, state in enumerate(T.run_reference(exe, d, case)):
            g = 0
            for si, progs in enumerate(systems):
                for ei, p in enumerate(progs):
                    n, eidx, rec, ch, rows, phys = state[g]
                    key = f"{case}/{k}/{g}/"
                    out[key + "counts"] = np.array([n, eidx], np.uint32)
                    out[key + "channels"] = np.ascontiguousarray(ch)
                    if phys is None:
                        out[key + "rows"] = rows.copy()
                    else:
                        L = options[si][ei].max_ribbon_length
                        out[key + "records"] = np.array(rec, np.uint32).reshape(-1, 3)
                        out[key + "rows"] = np.concatenate([phys[r * L:r * L + rec[r][1]] for r in range(len(rec))] + [np.zeros((0, p.outputs), np.float32)]).reshape(-1)
                    g += 1
    path = os.path.join(ROOT, "tests", "golden", "ribbons_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
