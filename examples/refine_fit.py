#!/usr/bin/env python3
"""PopPUNK's `--fit-model refine` on the device, on synthetic distances:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> BGMMModel.fit_dev: the first model, whose within / between component means start the search
    -> RefineBoundary.fit_dev: 40 boundaries along the line between the two means scored in one sweep, then scipy's
       bounded search between the best one's neighbours, every evaluation one device call on the resident matrix
       (ppk_refine_local_* between the two bound lines); then the core-only and accessory-only boundaries
                                                                                  PopPUNK/models.py:807-954
    -> save / from_npz: <prefix>/<prefix>_fit.npz with the reference's keys (no pickle)
    -> edge list of the refined boundary -> clusters = its connected components

    python examples/refine_fit.py [n_genomes] [strain_size] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import distfile, engine, models, network, refine, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_refine_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, member = synth.make_sketches(n, kmers, cluster_size=strain, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    names = ["genome%d" % k for k in range(n)]
    print("distances: %d pairs resident on the device" % dist_t.shape[0])

    bgmm = models.BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    print("BGMM fit: within-strain mean %s, between-strain mean %s (scaled)"
          % (np.round(bgmm.means[bgmm.within_label], 4), np.round(bgmm.means[bgmm.between_label], 4)))

    model = models.RefineBoundary()
    y = model.fit_dev(dist_t, names, bgmm, 0.0, 0.0, indiv_refine="both")
    info = refine.last_fit
    print("refined boundary: x_max %.5f, y_max %.5f (scaled); core-only %.5f, accessory-only %.5f (separately fitted: %s)"
          % (model.optimal_x, model.optimal_y, model.core_boundary, model.accessory_boundary, model.indiv_fitted))
    print("last search: %d evaluations scored through the %s path, rows base / candidates / never %s"
          % (len(info["evals"]), info["local_path"], info["split"]))

    path = model.save(os.path.join(work, "synthetic"))
    loaded = models.RefineBoundary.from_npz(path)
    scaled = dist_t / loaded.assign_dev(dist_t).new_tensor(loaded.scale)
    edges = engine.edge_threshold_dev(scaled, 2, loaded.optimal_x, loaded.optimal_y, inclusive=False).cpu().numpy()
    assert len(edges) == int((y == -1).sum().item())
    n_clusters, labels = distfile.clusters_from_edges(n, edges)
    numbers = network.cluster_numbers((np.asarray(edges, dtype=np.int64).reshape(-1, 2), n))
    print("PopPUNK's cluster numbers (printClusters: by size, largest first): %d clusters, the largest %d genomes"
          % (int(numbers.max()), int((numbers == 1).sum())))
    print("%s -> %d within-strain pairs -> %d clusters (%d synthetic strains)"
          % (path, len(edges), n_clusters, len(set(member.tolist()))))


if __name__ == "__main__":
    main()
