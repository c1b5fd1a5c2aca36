#!/usr/bin/env python3
"""PopPUNK's default `--fit-model bgmm` on the device, on synthetic distances:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> BGMMModel.fit_dev: subsample (or every row with max_samples=None), scale, the variational fit -- one pass over
       the training rows per iteration on the device, the M-step on the host -- assignment, within / between labels
                                                                                  PopPUNK/models.py:305-338
    -> save / from_npz: <prefix>/<prefix>_fit.npz with the reference's keys (no pickle)
    -> edges: every row labelled within-strain                                     PopPUNK/network.py:1170-1184
    -> clusters = connected components of the edge list

    python examples/bgmm_fit.py [n_genomes] [strain_size] [K] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import distfile, engine, models, network, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    work = sys.argv[4] if len(sys.argv) > 4 else tempfile.mkdtemp(prefix="ppk_bgmm_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, member = synth.make_sketches(n, kmers, cluster_size=strain, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    model = models.BGMMModel.fit_dev(dist_t, K, max_samples=None, seed=42)
    info = model.fit_info
    counts = np.bincount(model.labels.cpu().numpy(), minlength=K)
    print("fit on %d rows: run %d of %d won after %d iterations (converged: %s), bound %.4f; weights %s; within-strain "
          "label %d, between-strain label %d; rows per label %s"
          % (info["n_train"], info["best_init"], len(info["init_lower_bounds"]), info["n_iter"], info["converged"],
             info["lower_bound"], np.round(model.weights, 4), model.within_label, model.between_label, counts.tolist()))

    path = model.save(os.path.join(work, "synthetic"))
    loaded = models.BGMMModel.from_npz(path)
    edges = engine.bgmm_edges_dev(dist_t, loaded.model).cpu().numpy()
    assert len(edges) == counts[model.within_label]
    n_clusters, labels = distfile.clusters_from_edges(n, edges)
    numbers = network.cluster_numbers((np.asarray(edges, dtype=np.int64).reshape(-1, 2), n))
    print("PopPUNK's cluster numbers (printClusters: by size, largest first): %d clusters, the largest %d genomes"
          % (int(numbers.max()), int((numbers == 1).sum())))
    print("%s -> %d within-strain pairs -> %d clusters (%d synthetic strains)"
          % (path, len(edges), n_clusters, len(set(member.tolist()))))


if __name__ == "__main__":
    main()
