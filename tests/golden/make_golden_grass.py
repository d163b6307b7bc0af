"""Writes tests/golden/grass_small.npz: the maps of tests/test_gpu_grass.golden_scene() and what the REFERENCE's Terrain::createGrass and
renderGrass quad loop give for them - their code is cut out of the reference tree and compiled in a temporary directory by
tests/test_grass_oracle_vs_ref.py's harness; nothing of it is kept. The quads are stored in the device's list order (type, i, j); of every
pair of records the emplaced one is stored twice (the pushed copy's bytes depend on the reference's allocator). Needs the
reference tree; run from the repository root:

    python -m tests.golden.make_golden_grass
"""
import os
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def recorded(ref):
    """the fixture's arrays from the harness' records (tests/test_grass_oracle_vs_ref.run_ref)"""
    from tests import test_grass_oracle_vs_ref as T

    terrains, centres, positions, views = T.S.golden_scene()
    per_frame, per_view = T.run_ref(ref, terrains[0], [(7, centres[0], False)], positions[0], views)
    quads = per_frame[0]
    keys = sorted(quads)
    out = {"heightmap": np.ascontiguousarray(terrains[0]["heightmap"]), "splatmap": np.ascontiguousarray(terrains[0]["splatmap"])}
    heads = [quads[k][0] for k in keys]
    out["quad_aabb_min"] = np.array([h["aabb_min"] for h in heads], np.float32)
    out["quad_aabb_max"] = np.array([h["aabb_max"] for h in heads], np.float32)
    out["quad_ij"] = np.array([k[1:] for k in keys], np.int32)
    out["quad_type"] = np.array([k[0] for k in keys], np.uint32)
    out["quad_instances_count"] = np.array([h["instances_count"] for h in heads], np.uint32)
    inst = [np.repeat(np.ascontiguousarray(quads[k][1][0::2]).view(np.float32).reshape(-1, 8), 2, axis=0) for k in keys]
    out["instances"] = np.concatenate(inst).astype(np.float32)
    index = {k: n for n, k in enumerate(keys)}
    draws = sorted((v, index[(ti, i, j)], n, dist) for v, (_, _, _, ds) in enumerate(per_view) for ti, i, j, n, dist in ds)
    out["draw_view"] = np.array([d[0] for d in draws], np.uint32)
    out["draw_quad"] = np.array([d[1] for d in draws], np.uint32)
    out["draw_count"] = np.array([d[2] for d in draws], np.uint32)
    out["draw_distance"] = np.array([d[3] for d in draws], np.float32)
    out["culled"] = np.array([c for _, c, _, _ in per_view], np.uint32)
    return out


def main():
    from tests import test_grass_oracle_vs_ref as T

    with tempfile.TemporaryDirectory(prefix="lmx_grass_ref_") as d:
        out = recorded((T.build_harness(d), d))
    np.savez_compressed(os.path.join(HERE, "grass_small.npz"), **out)
    print(len(out["quad_type"]), "quads,", len(out["instances"]), "instance records,", len(out["draw_view"]), "draws, culled per view", out["culled"].tolist())


if __name__ == "__main__":
    main()
