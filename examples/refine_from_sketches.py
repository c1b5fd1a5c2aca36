#!/usr/bin/env python3
"""`--fit-model bgmm` then `--fit-model refine` through to weighted edges and clusters, without the [n_pairs, 2]
distance matrix at any step:

  SketchDB                                                    the sketches, resident                 engine.SketchDB
    -> BGMMModel.fit_from_sketches                              the start model, fitted on a subsample of pairs
    -> RefineBoundary.fit_from_sketches                         refine.refineFit driven by refine.SketchScorer: a few fused
                                                                passes (engine.dist_edges_rows) give the candidate pairs
                                                                with their distances; sweeps and the local search run on them
    -> boundary.edges_from_sketches(..., return_rows=True)      the fitted boundary's edges AND their distances, one pass
    -> engine.edge_weights_of_rows                              process_weights of that list, no further pass
    -> engine.mst_dev and engine.cluster_numbers_dev            the spanning forest and printClusters' numbers

    python examples/refine_from_sketches.py [n_genomes] [strain_size] [max_samples]          # needs an MI355X
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import engine, models, synth  # noqa: E402


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    max_samples = int(sys.argv[3]) if len(sys.argv) > 3 else 100000
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    db = engine.SketchDB(synth.make_sketches_device(n, kmers, cluster_size=strain, seed=7, device="cuda:0"), 16, 14)
    names = ["g%d" % k for k in range(n)]
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)

    bgmm = models.BGMMModel.fit_from_sketches(db, kmers, tbl, max_components=2, max_samples=max_samples, seed=42)
    boundary = models.RefineBoundary()
    boundary.fit_from_sketches(db, kmers, tbl, names, bgmm, 0.0, 0.0)
    print("refined boundary: core %.5f, accessory %.5f (scaled: %.4f, %.4f) after %d passes over the sketches"
          % (boundary.optimal_x * boundary.scale[0], boundary.optimal_y * boundary.scale[1], boundary.optimal_x,
             boundary.optimal_y, boundary.fit_passes))

    edges, rows, _ = boundary.edges_from_sketches(db, None, kmers, tbl, return_rows=True)
    weights = engine.edge_weights_of_rows(rows, "core")
    tree, components, _ = engine.mst_dev(edges, weights, n)
    numbers, n_clusters = engine.cluster_numbers_dev(edges, n)
    torch.cuda.synchronize()
    print("%d within-strain edges, weighted by core distance (%.5f .. %.5f); spanning forest of %d edges over %d "
          "components; %d clusters, the largest %d genomes"
          % (edges.shape[0], float(weights.min()), float(weights.max()), tree.shape[0], components, n_clusters,
             int((numbers == 1).sum())))
    # the library's scratch is grow-only, so what the steps took is still held
    print("device memory beyond the database: %.1f MB; the matrix would have taken %.1f MB"
          % ((free0 - torch.cuda.mem_get_info(0)[0]) / 1e6, n * (n - 1) // 2 * 8 / 1e6))


if __name__ == "__main__":
    main()
