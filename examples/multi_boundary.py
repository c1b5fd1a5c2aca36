#!/usr/bin/env python3
"""PopPUNK's `--fit-model refine --multi-boundary N` and `poppunk_iterate.py` on the device, on synthetic distances:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> BGMMModel.fit_dev: the first model, whose component means start the search
    -> RefineBoundary.fit_dev(multi_boundary=10, outPrefix=...): the refined boundary, then the clusters at 10
       boundaries between the axis and the optimum -- one sweep, one ppk_cluster_sweep_dev, and the
       <prefix>/<prefix>_boundary<k>_clusters.csv files printClusters writes          PopPUNK/refine.py:249-312
    -> iterate.iterate_clusters: the nested family of all those clusterings, every cluster's mean core distance from
       ONE pass over the matrix (ppk_cluster_pair_sums_dev), the tree and its cut     scripts/poppunk_iterate.py

    python examples/multi_boundary.py [n_genomes] [strain_size] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import engine, iterate, models, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_multi_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, member = synth.make_sketches(n, kmers, cluster_size=strain, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    names = ["genome%d" % k for k in range(n)]
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    bgmm = models.BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    prefix = os.path.join(work, "synthetic")
    model = models.RefineBoundary()
    model.fit_dev(dist_t, names, bgmm, 0.0, 0.0, multi_boundary=10, outPrefix=prefix)
    numbers, file_idx = model.multi_boundary_clusters
    print("refined boundary: x_max %.5f, y_max %.5f (scaled); boundary files %s, clusters per file %s"
          % (model.optimal_x, model.optimal_y, file_idx, numbers.max(axis=1).tolist()))

    res = iterate.iterate_clusters(os.path.join(prefix, "synthetic"), names, dist_t, cutoff=0.1,
                                   output=os.path.join(work, "synthetic_iterate"))
    top = res["sorted"][:5]
    print("family: %d clusters; the largest: %s"
          % (len(res["family"]), ", ".join("%d (%d genomes, Avg_Pi %.5f)" % (c, len(res["family"][c]), res["avg_pi"][c])
                                             for c in top)))
    print("cut at 0.1 of the largest Avg_Pi: %d clusters + %d singletons (%d synthetic strains); files under %s"
          % (len(res["cut_clusters"]), len(set(res["cut_assignment"].values())) - len(res["cut_clusters"]),
             len(set(member.tolist())), work))


if __name__ == "__main__":
    main()
