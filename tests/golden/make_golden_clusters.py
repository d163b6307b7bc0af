"""Writes tests/golden/clusters_small.npz: what the REFERENCE's PipelineImpl::fillClusters statements give for a small seeded scene - its
code is cut out of the reference tree and compiled in a temporary directory by tests/test_cluster_oracle_vs_ref.py's harness; nothing of it
is kept. Two views (128 x 64 and 200 x 130) of tests/cluster_oracle.scene(seed): the listed lights, a dozen probes of each kind (all
enabled, pairwise distinct volume products: DESIGN.md 4.11's deviations stay out), and per view the reference's planes, light records
(without the shadow-atlas slot, which is a table here), probe records, `clusters` and `map`. Needs the reference tree; run from the
repository root:

    python -m tests.golden.make_golden_clusters
"""
import os
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 5
VIEWS = ((128, 64), (200, 130))
N_LISTED = 240


def inputs():
    """-> (scene tables, listed entities, probe tables, views): everything a reader needs besides tests/cluster_oracle.scene(SEED)"""
    from tests import cluster_oracle as CO

    sc = CO.scene(SEED)
    listed = np.random.default_rng(SEED + 1).choice(CO.N_ENTITIES, N_LISTED, replace=False).astype(np.int32)
    probes = CO.probe_tables(12, 12, seed=SEED + 2, scene_seed=SEED, wide=(3,))
    return sc, listed, probes, [CO.view(w, h) for w, h in VIEWS]


def recorded(ref):
    from tests import test_cluster_oracle_vs_ref as T

    sc, listed, probes, views = inputs()
    out = {"kind": np.array("reference"), "seed": np.array(SEED), "listed": listed, "views": np.concatenate(views)}
    out.update({"probes_" + k: v for k, v in probes.items()})
    for i, view in enumerate(views):
        r = T.run_ref(ref, view, listed, sc["transforms"], sc["lights"], **probes)
        r["lights"]["atlas_idx"] = 0xFFFFFFFF  # (no atlas table: what the library and the oracle write then)
        out[f"v{i}_size"] = np.array(r["size"], np.int32)
        for k in ("xplanes", "yplanes", "zplanes", "lights", "env_probes", "refl_probes", "clusters", "map"):
            out[f"v{i}_{k}"] = r[k]
    return out


def main():
    from tests import test_cluster_oracle_vs_ref as T

    with tempfile.TemporaryDirectory(prefix="lmx_cluster_ref_") as d:
        out = recorded((T.build_harness(d), d))
    path = os.path.join(HERE, "clusters_small.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes;", [(out[f"v{i}_size"].tolist(), len(out[f"v{i}_map"])) for i in range(len(VIEWS))])


if __name__ == "__main__":
    main()
