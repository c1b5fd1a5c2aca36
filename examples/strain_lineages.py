#!/usr/bin/env python3
"""Lineages within every strain of a synthetic database, on the device:

  resident (core, accessory) matrix                              engine.dist
    -> a refine-style boundary and its within-strain edges       engine.edge_threshold_dev
    -> printClusters' numbers: the strains                       engine.cluster_numbers_dev
    -> the lineage model of EVERY strain from two calls over the resident matrix (every member's within-strain row
       sorted, lowerRank's rule for every rank) and one cluster sweep      lineages.fit_strain_lineages
    -> the id,Cluster,Rank_1,Rank_2,Rank_3,overall table of poppunk_lineages --create-db

    python examples/strain_lineages.py [n_genomes] [strain_size]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import engine, lineages, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    strain_size = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, _ = synth.make_sketches(n, kmers, cluster_size=strain_size, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    names = ["genome%03d" % k for k in range(n)]
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    # the boundary: between the within-strain and the between-strain distances
    x_max, y_max = synth.boundary_for_quantile(dist_t.cpu().numpy(), 0.9 * (strain_size - 1) / (n - 1))
    edges = engine.edge_threshold_dev(dist_t, 2, x_max, y_max)
    numbers, n_strains = engine.cluster_numbers_dev(edges, n)
    numbers = numbers.cpu().numpy()
    print("boundary (%.4f, %.4f): %d edges, %d strains" % (x_max, y_max, edges.shape[0], n_strains))

    # the strains as the clusters CSV gives them: string order, members in the file's row order (shuffled here)
    order = np.random.default_rng(3).permutation(n)
    strain_of = {}
    for k in order:
        strain_of.setdefault(str(numbers[k]), []).append(names[k])
    strain_of = {s: strain_of[s] for s in sorted(strain_of)}

    fitted = lineages.fit_strain_lineages(dist_t, names, strain_of, [1, 2, 3], min_count=10)
    print("%d strains of at least 10 genomes got lineages" % len(fitted))
    for strain, (model, clusters, overall) in list(fitted.items())[:5]:
        print("  strain %s: %d genomes, %d / %d / %d lineages at ranks 1 / 2 / 3, %d neighbour entries"
              % (strain, model.nn_dists.shape[0], max(clusters[1].values()), max(clusters[2].values()),
                 max(clusters[3].values()), model.nn_dists.nnz))
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "lineages.csv")
        lineages.print_overall_clustering({s: f[2] for s, f in fitted.items()}, table,
                                          [nm for s in fitted for nm in strain_of[s]])
        with open(table) as f:
            lines = f.read().splitlines()
    print("\n".join(lines[:6]))
    print("... %d rows" % (len(lines) - 1))
    assert lines[0] == "id,Cluster,Rank_1,Rank_2,Rank_3,overall"
    assert len(lines) - 1 == sum(len(strain_of[s]) for s in fitted)


if __name__ == "__main__":
    main()
