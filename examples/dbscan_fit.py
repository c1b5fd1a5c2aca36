#!/usr/bin/env python3
"""PopPUNK's `--fit-model dbscan` on the device, on synthetic distances:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> DBSCANModel.fit_dev: subsample, scale, core distances and the mutual-reachability spanning tree on the
       device, the HDBSCAN hierarchy on the host, within / between labels           PopPUNK/models.py:490-610
    -> save / from_npz: <prefix>_fit.npz with the reference's keys and this model's own arrays (no pickle)
    -> edges_dev: assign every row, keep the within-strain ones                      PopPUNK/network.py:1170-1184
    -> clusters = connected components of the edge list

    python examples/dbscan_fit.py [n_genomes] [strain_size] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import distfile, engine, models, network, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_dbscan_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, member = synth.make_sketches(n, kmers, cluster_size=strain)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    model = models.DBSCANModel()
    y = model.fit_dev(dist_t, max_num_clusters=10, min_cluster_prop=0.01, max_samples=3000, seed=7)
    counts = dict(zip(*np.unique(y.cpu().numpy(), return_counts=True)))
    print("fit: min_samples %d, min_cluster_size %d -> %d clusters; within-strain label %d, between-strain label %d; "
          "rows per label %s" % (model.min_samples, model.min_cluster_size, model.n_clusters, model.within_label,
                                 model.between_label, {int(k): int(v) for k, v in counts.items()}))

    path = model.save(os.path.join(work, "synthetic"))
    loaded = models.DBSCANModel.from_npz(path)
    edges = loaded.edges_dev(dist_t).cpu().numpy()
    assert len(edges) == counts.get(model.within_label, 0)
    n_clusters, labels = distfile.clusters_from_edges(n, edges)
    numbers = network.cluster_numbers((np.asarray(edges, dtype=np.int64).reshape(-1, 2), n))
    print("PopPUNK's cluster numbers (printClusters: by size, largest first): %d clusters, the largest %d genomes"
          % (int(numbers.max()), int((numbers == 1).sum())))
    print("%s -> %d within-strain pairs -> %d clusters (%d synthetic strains)"
          % (path, len(edges), n_clusters, len(set(member.tolist()))))


if __name__ == "__main__":
    main()
