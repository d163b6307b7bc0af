"""Records tests/golden/controllers_small.npz: the compiled reference's own results for the cases of tests/controller_cases.py (per case
the runtime data of every frame with SwitchNode's padding cleared, the blend stack after lmx_anim_decode_blend_stack with a clip's index as
its animation id, and root_motion). The reference is built as tests/test_controller_oracle_vs_ref.py builds it; without the reference
tree nothing is recorded.

    python -m tests.golden.make_golden_controllers
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import controller_cases as K  # noqa: E402
from tests import test_controller_oracle_vs_ref as R  # noqa: E402


def main():
    if not os.path.isdir(os.path.join(R.REF, "src")):
        raise SystemExit("no reference tree: the fixture records the compiled reference's results and nothing else")
    with tempfile.TemporaryDirectory() as d:
        results, lengths = R.run_reference(R.build_harness(d), d, K.CASES)
    assert lengths == [c["length"] for c in K.CLIPS]
    out = {}
    for c in K.CASES:
        _, frames = results[c["name"]]
        words = [R.switch_padding_mask(c, np.frombuffer(data, np.uint32)) for (data, _, _) in frames]
        instrs = [R.decoded(stack, c) for (_, stack, _) in frames]
        out[c["name"] + "/state"] = np.array([w for ws in words for w in ws], np.uint32)
        out[c["name"] + "/state_len"] = np.array([len(ws) for ws in words], np.uint32)
        out[c["name"] + "/instrs"] = np.concatenate(instrs).view(np.uint32)
        out[c["name"] + "/instr_len"] = np.array([len(i) for i in instrs], np.uint32)
        out[c["name"] + "/root_motion"] = np.array([rm for (_, _, rm) in frames], np.float32).view(np.uint32)
    path = os.path.join(ROOT, "tests", "golden", "controllers_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
