#!/usr/bin/env python3
"""How far the project's three models agree, and which levels of a boundary sweep really differ, by the adjusted Rand
index, on the device, on synthetic distances:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> a BGMM fit, a DBSCAN fit and a refine fit started from the BGMM, each to its within-strain edges and
       printClusters' numbers                                     models.*.fit_dev, network.cluster_numbers
    -> the Rand and adjusted Rand indices between the three clusterings (and the synthetic strains) from ONE call
       (ppk_contingency_sums_dev): every clustering against every clustering     scores.rand_of_levels
    -> a refine-style sweep of 12 boundaries                      engine.threshold_iterate_1d_dev, cluster_sweep_dev
    -> the level-by-level adjusted Rand matrix of the sweep from one more call, and which neighbouring levels are the
       same clustering

    python examples/rand_indices.py [n_genomes] [strain_size]          # needs an MI355X
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import engine, models, network, scores, synth  # noqa: E402


def numbers_of(edges, n):
    return network.cluster_numbers((np.asarray(edges, dtype=np.int64).reshape(-1, 2), n)).astype(np.int32)


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    n_off = 12
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, member = synth.make_sketches(n, kmers, cluster_size=strain, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    names = ["genome%d" % k for k in range(n)]
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    bgmm = models.BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    dbscan = models.DBSCANModel()
    dbscan.fit_dev(dist_t, max_num_clusters=10, min_cluster_prop=0.01, max_samples=3000, seed=7)
    refined = models.RefineBoundary()
    refined.fit_dev(dist_t, names, bgmm, 0.0, 0.0, indiv_refine=None)
    scaled = dist_t / dist_t.new_tensor(refined.scale)
    clusterings = {
        "bgmm": numbers_of(engine.bgmm_edges_dev(dist_t, bgmm.model).cpu().numpy(), n),
        "dbscan": numbers_of(dbscan.edges_dev(dist_t).cpu().numpy(), n),
        "refine": numbers_of(engine.edge_threshold_dev(scaled, 2, refined.optimal_x, refined.optimal_y,
                                                       inclusive=False).cpu().numpy(), n),
        "strains": scores.factorise(member.tolist())[0],
    }
    labels = list(clusterings)
    levels = torch.as_tensor(np.stack([clusterings[k] for k in labels]), device=dist_t.device)
    rand, adjusted, refines = scores.rand_of_levels(levels)
    print("clusters: " + ", ".join("%s %d" % (k, int(len(np.unique(v)))) for k, v in clusterings.items()))
    print("adjusted Rand index (above the diagonal) and Rand index (below):")
    print("          " + "".join("%9s" % k for k in labels))
    for x, k in enumerate(labels):
        print("%9s " % k + "".join("%9.4f" % (1.0 if x == y else adjusted[x, y] if x < y else rand[x, y])
                                   for y in range(len(labels))))
    for x, kx in enumerate(labels):
        for y, ky in enumerate(labels):
            if x != y and refines[x, y]:
                print("  every %s cluster lies inside one %s cluster" % (kx, ky))
    # sklearn's signature gives the same float from the host arrays
    assert scores.adjusted_rand_score(clusterings["bgmm"].tolist(), clusterings["dbscan"].tolist()) == adjusted[0, 1]

    # the sweep: boundaries of slope 2 from the 1 % to the 50 % quantile point of the scaled distances
    xs = (dist_t / dist_t.amax(dim=0)).contiguous()
    sample = xs.cpu().numpy()
    m0, m1 = np.quantile(sample, 0.01, axis=0), np.quantile(sample, 0.50, axis=0)
    offsets = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), n_off), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offsets, 2, m0[0], m0[1], m1[0], m1[1])
    levels_t, counts_t = engine.cluster_sweep_dev(i, j, o, n, n_off)
    counts = counts_t.cpu().numpy()
    _, adjusted, refines = scores.rand_of_levels(levels_t)
    print("boundary sweep, adjusted Rand index of level against level (clusters per level %s):" % counts.tolist())
    for x in range(n_off):
        print("  %2d " % x + " ".join("%5.2f" % v for v in adjusted[x]))
    same = [t for t in range(n_off - 1) if adjusted[t, t + 1] == 1.0]
    print("neighbouring levels that are the same clustering: %s" % (same if same else "none"))
    assert all(refines[x, y] for x in range(n_off) for y in range(x, n_off))      # a sweep's graphs only grow


if __name__ == "__main__":
    main()
