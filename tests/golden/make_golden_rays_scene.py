"""Writes tests/golden/rays_scene_small.npz: the inputs of tests/test_gpu_rays_scene.golden_scene() and the records the REFERENCE's
castRayProceduralGeometry, Terrain::castRay and castRay tail give for them - its code is cut out of the reference tree and compiled in a
temporary directory by tests/test_ray_scene_oracle_vs_ref.py's harness; nothing of it is kept. castRay(ray, ignored) knows no t_max: the
merged hit is kept where it is below the ray's t_max (the caller's `held` rule), the two stages' own records are kept as they are. Needs
the reference tree; run from the repository root:

    python -m tests.golden.make_golden_rays_scene
"""
import os
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def recorded(sc, rays, pg, th, fin):
    """the fixture's arrays from the harness' records (tests/test_ray_scene_oracle_vs_ref.run_ref)"""
    from tests.test_ray_scene_oracle_vs_ref import COMPONENT

    out = {"rays": np.ascontiguousarray(rays).view(np.uint8), "transforms": np.ascontiguousarray(sc["transforms"]).view(np.uint8)}
    for k, t in enumerate(sc["terrains"]):
        out[f"heightmap{k}"] = np.ascontiguousarray(t["heightmap"])
    for k, g in enumerate(sc["pg"]):
        out[f"vertex_data{k}"] = np.ascontiguousarray(g["vertex_data"])
    out["pg_is_hit"], out["pg_entity"], out["pg_t"] = pg["is_hit"].astype(np.uint32), pg["entity"].astype(np.int32), pg["t"].astype(np.float32)
    entities = np.array([int(t["entity"]) for t in sc["terrains"]], np.int32)
    out["terrain_is_hit"], out["terrain_t"] = th["is_hit"].astype(np.uint32), th["t"].astype(np.float32)
    out["terrain_entity"] = np.where(th["is_hit"] == 1, entities[None, :], 0).astype(np.int32)  # (Terrain::castRay leaves the entity to its caller, :2771)
    held = (fin["is_hit"] == 1) & (fin["t"] < rays["t_max"])
    back = {v: k for k, v in COMPONENT.items()}
    out["scene_is_hit"] = held.astype(np.uint32)
    out["scene_component"] = np.array([back[int(c)] if h else 0 for c, h in zip(fin["component"], held)], np.uint32)
    out["scene_entity"] = np.where(held, fin["entity"], 0).astype(np.int32)
    out["scene_t"] = np.where(held, fin["t"], 0).astype(np.float32)
    return out


def main():
    from tests import test_ray_scene_oracle_vs_ref as T

    sc, rays = T.S.golden_scene()
    with tempfile.TemporaryDirectory(prefix="lmx_ray_scene_ref_") as d:
        _, (pg, th, fin) = T.reference_records((T.build_harness(d), d), sc, rays)
    out = recorded(sc, rays, pg, th, fin)
    np.savez_compressed(os.path.join(HERE, "rays_scene_small.npz"), **out)
    print(int(out["pg_is_hit"].sum()), "procedural,", int(out["terrain_is_hit"].sum()), "terrain and", int(out["scene_is_hit"].sum()), "merged hits of", len(rays), "rays")


if __name__ == "__main__":
    main()
