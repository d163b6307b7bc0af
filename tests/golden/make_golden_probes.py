"""Records tests/golden/probes_small.npz: the reference's own outputs for every case of tests/probe_oracle.cases().

    python -m tests.golden.make_golden_probes          (where the reference tree exists)

SphericalHarmonics and saveCubemap's RGBM lines are compiled out of the reference by the harness of tests/test_probe_oracle_vs_ref.py
(nothing of it is committed) and run on each case. Keys are "<case>|<array>": `sh` (n, 9, 3) for every case; `mip1` ... for the cases
with a chain (the harness's restatement of the `downscale` loop); "rgbm routes|rgbm", the bytes of the clamp-route cubemap. The inputs
are not stored: probe_oracle.cases() builds them from fixed seeds.

`e32` (n, 4) is not the reference's: per probe and level 1 .. 4 the largest difference between the oracle's radiance level in float32
and in float64, divided by the level's largest value - the unit of the device's bound in tests/test_gpu_probes.py.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def e32_of(cubemap):
    from tests import probe_oracle as PO

    lo, hi = PO.filter_levels(cubemap), PO.filter_levels(cubemap, T=np.float64)
    return np.array([np.abs(lo[k][..., :3].astype(np.float64) - hi[k][..., :3]).max() / np.abs(hi[k][..., :3]).max() for k in range(1, 5)])


def recorded(ref):
    from tests import probe_oracle as PO
    from tests.test_probe_oracle_vs_ref import ref_mips, ref_rgbm, ref_sh

    out = {}
    for name, c in PO.cases().items():
        out[f"{name}|sh"] = np.stack([ref_sh(ref, p) for p in c["cubemaps"]])
        if c["mips"]:
            chains = [ref_mips(ref, p) for p in c["cubemaps"]]
            for m in range(len(chains[0])):
                out[f"{name}|mip{m + 1}"] = np.stack([ch[m] for ch in chains])
        if c.get("filter"):
            out[f"{name}|e32"] = np.stack([e32_of(p) for p in c["cubemaps"]])
    out["rgbm routes|rgbm"] = ref_rgbm(ref, PO.rgbm_routes())
    return out


if __name__ == "__main__":
    from tests.test_probe_oracle_vs_ref import GOLDEN, build_harness

    with tempfile.TemporaryDirectory() as d:
        work = os.path.join(d, "ref")
        os.makedirs(work)
        np.savez_compressed(GOLDEN, **recorded((build_harness(work), work)))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
