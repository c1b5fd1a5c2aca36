#!/usr/bin/env python3
"""`--fit-model bgmm` through to a weighted network without the [n_pairs, 2] distance matrix:

  SketchDB                                                    the sketches, resident                 engine.SketchDB
    -> BGMMModel.fit_from_sketches: the training rows (models.sample_rows) as a pair list, their distances from
       the sketches (engine.dist_pairs), the fit of models.py:305-338 on that subsample
    -> model.edges_from_sketches: kernel 1 fused with the model's label test, edges only
    -> engine.edge_weights_from_sketches: process_weights of that list, again from the sketches
                                                                PopPUNK/network.py:646-674, scripts/poppunk_add_weights.py
    -> engine.mst_dev (generate_minimum_spanning_tree) and engine.cluster_numbers_dev (printClusters)

    python examples/matrix_free_fit.py [n_genomes] [strain_size] [max_samples]          # needs an MI355X
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
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    low = [free0]

    def mark():
        torch.cuda.synchronize()
        low.append(torch.cuda.mem_get_info(0)[0])

    model = models.BGMMModel.fit_from_sketches(db, kmers, tbl, max_components=2, max_samples=max_samples, seed=42)
    mark()
    info = model.fit_info
    print("fit on %d of %d rows: %d iterations, weights %s, within-strain label %d"
          % (info["n_train"], n * (n - 1) // 2, info["n_iter"], np.round(model.weights, 4), model.within_label))

    edges, _ = model.edges_from_sketches(db, None, kmers, tbl)
    mark()
    weights = engine.edge_weights_from_sketches(db, None, kmers, tbl, edges, "core")
    mark()
    tree, components, _ = engine.mst_dev(edges, weights, n)
    numbers, n_clusters = engine.cluster_numbers_dev(edges, n)
    mark()
    print("%d within-strain edges, weighted by core distance (%.5f .. %.5f); spanning forest of %d edges over %d "
          "components; %d clusters, the largest %d genomes"
          % (edges.shape[0], float(weights.min()), float(weights.max()), tree.shape[0], components, n_clusters,
             int((numbers == 1).sum())))
    # free memory is sampled between the steps; the library's scratch is grow-only, so what a step took is still held
    print("device memory beyond the database: %.1f MB at most between steps; the matrix would have taken %.1f MB"
          % ((free0 - min(low)) / 1e6, n * (n - 1) // 2 * 8 / 1e6))


if __name__ == "__main__":
    main()
