"""Writes tests/golden/animcomp_small.npz: a handful of the clips of tests/animcomp_cases.py and, for each, the bytes the reference's own
write_animation leaves from the translation count on (tests/test_animcomp_oracle_vs_ref.py's harness; needs the reference tree).

    python -m tests.golden.make_golden_animcomp
"""
import os
import tempfile

import numpy as np

from tests import animcomp_cases as AC
from tests import test_animcomp_oracle_vs_ref as R

NAMES = ("2 samples", "65 samples, 3 bones", "frame of 4 bits", "57 bits at offset 7 (& 7 = 7)", "zeros in different workgroups, 1 bone", "clamp, one largest", "clamp, four equal sizes",
         "leaves the bind pose in its last sample", "ties at k + 0.5", "63 samples, 64 bones")

if __name__ == "__main__":
    work = tempfile.mkdtemp()
    exe = R.build_harness(work)
    clips = [AC.by_name(n) for n in NAMES]
    got, _ = R.ref_run(exe, work, clips, R.HASHES)
    out = {"names": np.array(NAMES)}
    for i, (c, (asserts, data)) in enumerate(zip(clips, got)):
        assert asserts == 0
        out[f"keys_{i}"], out[f"bind_{i}"], out[f"bytes_{i}"] = AC.as_floats(c["keys"]), c["bind"], np.frombuffer(data, np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "animcomp_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
