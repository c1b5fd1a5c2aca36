#!/usr/bin/env python3
"""The end of a model fit on the device, on synthetic genomes: which genomes does the reference database keep?

  a database of synthetic genomes -> distances -> a boundary -> the network's edges (the fused path of the fit)
    -> network.extractReferences: reference genomes per cluster by clique pruning and path repair, the .refs file
       and the network among the references (ppk_pick_refs_dev)        PopPUNK/network.py:283-509, DESIGN.md 3.25
    -> the reference database: the references' sketches alone, their network's component labels
    -> every genome that was left out assigned back as a query (the fused query-reference edges and ONE
       ppk_cluster_extend_dev): the clusters of all genomes are those of the full network

    python examples/pick_references.py [n_genomes] [strain_size] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import assign, engine, models, network, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1200
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_refs_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sketches, _ = synth.make_sketches(n, kmers, cluster_size=strain, seed=11)
    names = ["genome%04d" % k for k in range(n)]

    db = engine.SketchDB(np.ascontiguousarray(sketches), 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    x_max, y_max = synth.boundary_for_quantile(dist[::7].cpu().numpy(), 0.6 * (strain - 1) / (n - 1))
    del dist
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max)
    edges, _ = model.edges_from_sketches(db, None, kmers, tbl)
    db.close()
    full, n_clusters = engine.cluster_numbers_dev(edges, n)
    print("network: %d genomes, %d edges, %d clusters" % (n, edges.shape[0], n_clusters))

    out = os.path.join(work, "refs")
    os.makedirs(out, exist_ok=True)
    idx, ref_names, ref_file, G_ref = network.extractReferences((edges, n), names, out)
    print("references: %d genomes, %d edges among them; %s" % (len(idx), G_ref[0].shape[0], ref_file))

    rest = np.setdiff1d(np.arange(n), idx)
    ref_db = engine.SketchDB(np.ascontiguousarray(sketches[idx]), 16, 14, device=0)
    qry_db = engine.SketchDB(np.ascontiguousarray(sketches[rest]), 16, 14, device=0)
    q_edges, _ = model.edges_from_sketches(ref_db, qry_db, kmers, tbl)
    ref_db.close()
    qry_db.close()
    numbers, n_back = engine.cluster_extend_dev(q_edges, assign.component_labels(G_ref), len(rest))
    back = np.empty(n, dtype=np.int64)
    back[np.concatenate([idx, rest])] = numbers.cpu().numpy()
    first_full, first_back = {}, {}
    full = full.cpu().numpy()
    same = all(first_full.setdefault(int(a), v) == first_back.setdefault(int(b), v) for v, (a, b) in enumerate(zip(full, back)))
    print("assigned back: %d queries against %d references -> %d clusters, %s the full network's"
          % (len(rest), len(idx), n_back, "the same partition as" if same else "NOT"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
