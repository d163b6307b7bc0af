"""Writes tests/golden/texmips_small.npz from the reference (needs its tree and g++): per size of
tests/test_texmips_oracle_vs_ref.py's FIXTURE_SIZES three images (noise, a smooth ramp, a block of zero alpha), the reference's chains in
each mode without and with coverage scaling, its coverage of image 0, and the measured shares of bytes at which tests/texmips_oracle.py's
filtered levels differ from stb's.

    python -m tests.golden.make_golden_texmips
"""
import os
import tempfile

import numpy as np

from tests import test_texmips_oracle_vs_ref as R

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as work:
        data = R.recorded((R.build_harness(work), work))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "texmips_small.npz")
    np.savez_compressed(out, **data)
    for mode in ("linear", "srgb"):
        n, differ = data[f"share_{mode}"]
        print(f"{mode}: {differ} of {n} bytes differ from stb's ({100.0 * differ / n:.4f} %)")
    print(out, os.path.getsize(out), "bytes")
