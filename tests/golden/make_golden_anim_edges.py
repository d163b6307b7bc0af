"""Writes tests/golden/anim_edges.npz: what the REFERENCE's own sampler (AnimationSampler::getRelativePose, sliced out of the reference tree
into oracle/_ref at build time, oracle/ref/anim_shim.cpp) gives for the layout and the clip-end cases of tests/anim_cases.py - the poses and
new times of every lmx_anim_update run of the case, the poses of its blend stacks and of its programs with IK. tests/test_anim_edges.py holds
the port oracle to it, tests/test_gpu_anim_edges.py the device, also where oracle/_ref is not built or comes from an older shim. Needs the
reference oracle, built from this tree's shim (checked); run from the repository root:

    python -m tests.golden.make_golden_anim_edges
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from oracle import pyoracle
    from tests import anim_cases as AC

    pyoracle.build()  # make: brings oracle/_ref up to this tree's shims
    ref = pyoracle.Oracle("reference")
    if not ref.anim_pads_root_motion():
        raise SystemExit("oracle/_ref/liblmx_ref.so comes from an older oracle/ref/anim_shim.cpp: its sampler reads behind the root-motion vectors at a clip's end. "
                         "Rebuild it from this tree (oracle.pyoracle.build(force=True)) before recording.")
    out = {}
    for case in AC.all_cases():
        if case.golden:
            out.update(AC.record(ref, case))
    path = os.path.join(HERE, "anim_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
