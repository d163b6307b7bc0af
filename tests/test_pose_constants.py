"""api.POSE_BLOCK / POSE_GRID / POSE_DQ_GRID mirror the launch geometry of pose_kernels.hip (lmx_kernels.h). tests/test_gpu_pose_lists.py
computes every wave, tile and block edge it lists from the mirrors: retuned kernels either move those tests along or fail here."""
import os
import re

from lumixengine_amd import api

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lumixengine_amd", "csrc", "lmx_kernels.h")


def test_pose_launch_geometry_mirrors_the_header():
    text = open(HEADER).read()
    for name in ("POSE_BLOCK", "POSE_GRID", "POSE_DQ_GRID"):
        found = re.findall(r"^constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)u?\s*;", text, re.M)
        assert len(found) == 1, f"{name}: expected one `constexpr uint32_t {name} = <literal>;` in lmx_kernels.h, found {len(found)}"
        assert int(found[0]) == getattr(api, name), f"api.{name} = {getattr(api, name)}, lmx_kernels.h says {found[0]}"
