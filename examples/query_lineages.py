#!/usr/bin/env python3
"""Both modes of poppunk_lineages on a synthetic database, on the device:

  a sketched reference database, its stored distances, its fitted boundary and its strains (what a fit leaves behind)
    -> python -m poppunk_amd.lineages --create-db : the lineage model of EVERY strain from one pass over the matrix
                                                                            lineages.create_db, DESIGN.md 3.21
  a sketched query database
    -> python -m poppunk_amd.lineages --query-db  : query x reference and query x query distances, the strain of every
       query (assign.assign_query_clusters), then the queries merged into the stored neighbour lists of ALL their
       strains in one call, lowerRank's rule for every rank and one cluster sweep
                                                                            lineages.query_db, DESIGN.md 3.22
    -> <output>.csv: id,Cluster,Rank_1,Rank_2,Rank_3,overall for the queries

    python examples/query_lineages.py [n_references] [n_queries] [strain_size] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import distfile, engine, lineages, models, network, sketchdb, synth  # noqa: E402


def main():
    n_ref = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    n_qry = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    strain_size = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    work = sys.argv[4] if len(sys.argv) > 4 else tempfile.mkdtemp(prefix="ppk_lineages_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    # the queries are drawn evenly across the genomes, so every strain gives a few
    n = n_ref + n_qry
    sketches, _ = synth.make_sketches(n, kmers, cluster_size=strain_size, seed=7)
    is_query = np.zeros(n, dtype=bool)
    is_query[np.linspace(0, n - 1, n_qry).astype(np.int64)] = True
    rNames = ["ref%03d" % k for k in range(n_ref)]
    qNames = ["query%03d" % k for k in range(n_qry)]
    os.chdir(work)
    sketchdb.save_npz(os.path.join("db", "db"), rNames, kmers, sketches[~is_query], 16, 14, random_table=tbl)
    sketchdb.save_npz(os.path.join("queries", "queries"), qNames, kmers, sketches[is_query], 16, 14, random_table=tbl)

    # what the fit left behind: the stored distances, a boundary, the strains under it
    ref_db = engine.SketchDB(np.ascontiguousarray(sketches[~is_query]), 16, 14, device=0)
    rr, _ = engine.dist(ref_db, None, kmers, tbl)
    ref_db.close()
    X = rr.cpu().numpy()
    distfile.storePickle(rNames, rNames, True, X, os.path.join("db", "db.dists"))
    x_max, y_max = synth.boundary_for_quantile(X, 0.9 * (strain_size - 1) / (n - 1))
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max, core_boundary=x_max,
                                  accessory_boundary=y_max)
    model.save("db")
    edges = engine.edge_threshold_dev(rr, 2, x_max, y_max)
    network.printClusters((edges, n_ref), rNames, outPrefix=os.path.join("db", "db"), write_unwords=False)
    print("references: %d genomes, %d within-strain edges; work directory %s" % (n_ref, edges.shape[0], work))

    lineages.main(["--create-db", "db", "--db-scheme", "scheme.pkl", "--output", "references", "--overwrite"])
    lineages.main(["--query-db", "queries", "--db-scheme", "scheme.pkl", "--output", "assigned"])
    with open("assigned.csv") as f:
        lines = f.read().splitlines()
    print("\n".join(lines[:6]))
    print("... %d of %d queries are in a strain that has lineages" % (len(lines) - 1, n_qry))
    assert lines[0] == "id,Cluster,Rank_1,Rank_2,Rank_3,overall"
    assert 0 < len(lines) - 1 <= n_qry and all(line.startswith("query") for line in lines[1:])


if __name__ == "__main__":
    main()
