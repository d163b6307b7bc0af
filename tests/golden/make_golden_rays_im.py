"""Writes tests/golden/rays_im_small.npz: the inputs of tests/test_gpu_rays_im.golden_scene() and the hits the REFERENCE's
castRayInstancedModels gives for them, kept where they are below the ray's t_max (the caller's `held` rule) - its code is cut out of the
reference tree and compiled in a temporary directory by tests/test_ray_im_oracle_vs_ref.py's harness; nothing of it is kept. Needs the
reference tree; run from the repository root:

    python -m tests.golden.make_golden_rays_im
"""
import os
import tempfile

import numpy as np

from tests import test_ray_im_oracle_vs_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sc, models, rays = T.S.golden_scene()
    out = {"n_meshes": np.int32(len(sc["meshes"])), "models": np.ascontiguousarray(sc["models"]).view(np.uint8), "rays": np.ascontiguousarray(rays).view(np.uint8),
           "n_im_models": np.int32(len(models)), "im_ray_model": np.array([m["ray_model"] for m in models], np.int32),
           "im_entity": np.array([m["entity"] for m in models], np.int32), "im_origin": np.array([m["origin"] for m in models], np.float64)}
    for k, m in enumerate(sc["meshes"]):
        out[f"mesh{k}_positions"], out[f"mesh{k}_indices"] = m["positions"], m["indices"]
    for k, m in enumerate(models):
        out[f"im{k}_instances"] = np.ascontiguousarray(m["instances"]).view(np.uint8)  # (as given; the device puts them into grid order)
    sc = T.stored(sc, models)
    with tempfile.TemporaryDirectory(prefix="lmx_ray_im_ref_") as d:
        hits = T.run_ref(T.build_harness(d), d, sc, rays)
    assert T.RIO.agrees(sc, rays)
    held = hits["is_hit"].astype(bool) & (hits["t"] < rays["t_max"])
    for k in ("is_hit", "entity", "subindex", "mesh", "t"):
        out["hit_" + k] = np.where(held, hits[k], 0).astype(hits[k].dtype)
    np.savez_compressed(os.path.join(HERE, "rays_im_small.npz"), **out)
    print(int(held.sum()), "of", len(rays), "rays hit")


if __name__ == "__main__":
    main()
