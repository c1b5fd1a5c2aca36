#!/usr/bin/env python3
"""Ranking the clusterings of a boundary sweep by their silhouette, on the device, on synthetic distances:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> a refine-style sweep of 20 boundaries across the within / between gap     engine.threshold_iterate_1d_dev
    -> printClusters' numbers of every genome in every graph of the sweep        engine.cluster_sweep_dev
    -> the mean silhouette of every level from ONE call on the matrix (ppk_silhouette_dev), NaN where a level has
       fewer than 2 or more than n - 1 clusters                                  scores.silhouette_of_levels
    -> the best level's clusters, and the score scripts/poppunk_calculate_silhouette.py would print for them

    python examples/silhouette.py [n_genomes] [strain_size]          # needs an MI355X
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import engine, scores, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    n_off = 20
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, member = synth.make_sketches(n, kmers, cluster_size=strain, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    # the sweep: boundaries of slope 2 from the 1 % to the 50 % quantile point of the scaled distances
    xs = (dist_t / dist_t.amax(dim=0)).contiguous()
    sample = xs.cpu().numpy()
    m0, m1 = np.quantile(sample, 0.01, axis=0), np.quantile(sample, 0.50, axis=0)
    offsets = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), n_off), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offsets, 2, m0[0], m0[1], m1[0], m1[1])
    levels_t, counts_t = engine.cluster_sweep_dev(i, j, o, n, n_off)
    counts = counts_t.cpu().numpy()

    means = scores.silhouette_of_levels(dist_t, levels_t, metric="euclidean")
    for t in range(n_off):
        print("  boundary %2d: %4d clusters, mean silhouette %s"
              % (t, counts[t], "-- (not scored)" if np.isnan(means[t]) else "%.4f" % means[t]))
    if np.all(np.isnan(means)):
        print("no level of the sweep has between 2 and n - 1 clusters")
        return
    best = int(np.nanargmax(means))
    numbers = levels_t[best].cpu().numpy()
    sizes = np.bincount(numbers)[1:]
    print("best: boundary %d, %d clusters (%d synthetic strains), largest %s"
          % (best, counts[best], len(set(member.tolist())), sizes[:5].tolist()))
    # the same score through sklearn's signature, from the long-form matrix on the host
    score = scores.silhouette_score(dist_t.cpu().numpy(), numbers.tolist(), metric="euclidean")
    assert score == means[best]
    print("scores.silhouette_score of that clustering: %.6f" % score)


if __name__ == "__main__":
    main()
