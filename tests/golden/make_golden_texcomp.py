"""Records tests/golden/texcomp_small.npz: the reference's own encoder on the blocks of tests/texcomp_oracle.fixture_blocks().

    python -m tests.golden.make_golden_texcomp          (where the reference tree exists)

The harness of tests/test_texcomp_oracle_vs_ref.py is built around the reference's external/rgbcx/rgbcx.h in a temporary directory (nothing
of it is committed). Keys: `rgba` (N, 16, 4), the blocks; `l10_4` / `l10_3`, the level-10 bytes without / with 3-colour blocks; `ex_4` /
`ex_3`, the exhaustive mode's; each with `_err`, the squared RGB difference under the ideal decode (tests/texcomp_oracle.decode_bc1);
`bc4` (channel 0) and `bc5`, encode_bc4's and encode_bc5's bytes.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from tests import texcomp_oracle as TO
    from tests.test_texcomp_oracle_vs_ref import GOLDEN, build_harness, recorded

    blocks = TO.fixture_blocks()
    TO.encode_bc1(blocks, True)  # the routes the fixture is meant to take
    assert TO.STATS["clamped"] > 0 and TO.STATS["det0"] > 0, TO.STATS
    with tempfile.TemporaryDirectory() as d:
        np.savez_compressed(GOLDEN, **recorded((build_harness(d), d), blocks))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(blocks), "blocks,", TO.STATS)
