"""Records tests/golden/voxels_small.npz: the reference's own outputs for every case of tests/voxel_oracle.cases().

    python -m tests.golden.make_golden_voxels          (where the reference tree exists)

Voxels is compiled out of the reference by the harness of tests/test_voxel_oracle_vs_ref.py (nothing of it is committed) and run on each
case: per case the inputs (vertex and index arrays, the box or max_res, the ray counts, the seed, the lookup points) and what the
reference gave - grid, voxel bytes, AO behind every computeAO with the generator's state, lookups, blurred AO, baked bytes. Keys are
"<case>|<array>". tests/test_voxels_cpu.py and tests/test_gpu_voxels.py compare against it without the reference;
test_voxel_oracle_vs_ref.py checks that the committed file is still what the reference gives.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def recorded(ref):
    from tests import voxel_oracle as VO
    from tests.test_voxel_oracle_vs_ref import run_ref

    out = {}
    for name, c in VO.cases().items():
        for k, v in run_ref(ref, c).items():
            out[f"{name}|{k}"] = np.asarray(v)
        for m, (p, i) in enumerate(c["meshes"]):
            out[f"{name}|positions{m}"] = np.ascontiguousarray(p, np.float32)
            out[f"{name}|indices{m}"] = np.ascontiguousarray(i)
        out[f"{name}|max_res"] = np.array([c["max_res"]], np.uint32)
        out[f"{name}|ray_counts"] = np.array(c["ao"], np.uint32)
        out[f"{name}|seed"] = np.array(c["seed"], np.uint32)
        if c["begin"] is not None:
            out[f"{name}|begin"] = np.asarray(c["begin"], np.float32)
    return out


if __name__ == "__main__":
    from tests.test_voxel_oracle_vs_ref import GOLDEN, build_harness

    with tempfile.TemporaryDirectory() as d:
        work = os.path.join(d, "ref")
        os.makedirs(work)
        np.savez_compressed(GOLDEN, **recorded((build_harness(work), work)))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
