"""Writes tests/golden/rays_small.npz: the inputs of tests/test_ray_oracle_vs_ref.golden_scene() and the hits the REFERENCE's castRay loop
gives for them - its code is cut out of the reference tree and compiled in a temporary directory by that test module's harness; nothing
of it is kept. Needs the reference tree; run from the repository root:

    python -m tests.golden.make_golden_rays
"""
import os
import tempfile

import numpy as np

from tests import test_ray_oracle_vs_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sc, rays = T.golden_scene()
    with tempfile.TemporaryDirectory(prefix="lmx_ray_ref_") as d:
        hits, _ = T.run_ref(T.build_harness(d), d, sc, rays)
    assert T.RO.agrees(sc, rays)
    out = {"n_meshes": np.int32(len(sc["meshes"])), "models": np.ascontiguousarray(sc["models"]).view(np.uint8), "inst_model": sc["inst_model"],
           "inst_flags": sc["inst_flags"], "transforms": np.ascontiguousarray(sc["transforms"]).view(np.uint8), "rays": np.ascontiguousarray(rays).view(np.uint8)}
    for k, m in enumerate(sc["meshes"]):
        out[f"mesh{k}_positions"], out[f"mesh{k}_indices"] = m["positions"], m["indices"]
    for k in ("is_hit", "entity", "mesh", "t"):
        out["hit_" + k] = hits[k]
    np.savez_compressed(os.path.join(HERE, "rays_small.npz"), **out)
    print(int(hits["is_hit"].sum()), "of", len(rays), "rays hit")


if __name__ == "__main__":
    main()
