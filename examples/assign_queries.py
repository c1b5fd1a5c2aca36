#!/usr/bin/env python3
"""`poppunk_assign`'s last step on the device, on synthetic genomes: which cluster is every new genome in?

  a reference database, its fitted boundary, its network and its cluster file (what a fit leaves behind)
    -> assign.ReferenceNetwork: the component label of every reference, computed once and kept on the device
    -> assign.assign_from_sketches: the fused distance -> edge path for the query-reference pairs (the matrix is never
       formed), every query's degree (ppk_query_links_dev), query-query edges if a query is unlinked, ONE
       ppk_cluster_extend_dev over the new edges, and printClusters' names against the old cluster file
                                                        PopPUNK/assign.py:592-660, network.py:1315-1442, 1478-1663
    -> engine.query_links_dev on the same edges: how many old clusters every query touches (the graph QC of
       qc.qcQueryAssignments, and what `--serial` names a query from)
    -> network.vertex_betweenness on the network after assignment: `poppunk_assign --betweenness`'s table
                                                        PopPUNK/assign.py:646-651

    python examples/assign_queries.py [n_references] [n_queries] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import assign, engine, models, network, synth  # noqa: E402


def main():
    n_ref = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    n_qry = int(sys.argv[2]) if len(sys.argv) > 2 else 120
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_assign_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sketches, _ = synth.make_sketches(n_ref + n_qry, kmers, cluster_size=30, seed=7)
    ref_db = engine.SketchDB(np.ascontiguousarray(sketches[:n_ref]), 16, 14, device=0)
    qry_db = engine.SketchDB(np.ascontiguousarray(sketches[n_ref:]), 16, 14, device=0)
    rNames = ["ref%d" % k for k in range(n_ref)]
    qNames = ["query%d" % k for k in range(n_qry)]

    # what the fit left behind: a boundary, the network of the references under it, its clusters
    rr, _ = engine.dist(ref_db, None, kmers, tbl)
    x_max, y_max = synth.boundary_for_quantile(rr[::7].cpu().numpy(), 0.03)
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max)
    ref_edges, _ = model.edges_from_sketches(ref_db, None, kmers, tbl)
    del rr
    fit = os.path.join(work, "fit")
    os.makedirs(fit, exist_ok=True)
    network.printClusters((ref_edges, n_ref), rNames, outPrefix=os.path.join(fit, "fit"), write_unwords=False)
    refnet = assign.ReferenceNetwork((ref_edges, n_ref), rNames, os.path.join(fit, "fit_clusters.csv"))
    print("reference network: %d genomes, %d edges, %d clusters" % (n_ref, ref_edges.shape[0],
                                                                   len(set(refnet.labels.tolist()))))

    out = os.path.join(work, "assigned")
    os.makedirs(out, exist_ok=True)
    clustering, merged = assign.assign_from_sketches(ref_db, qry_db, model, refnet, qNames, kmers, tbl, out)
    names = [clustering[q] for q in qNames]
    old = set(clustering[r] for r in rNames)
    print("queries: %d in an existing cluster, %d in new clusters, %d in a merged cluster; %s"
          % (sum(c in old and "_" not in c for c in names), sum(c not in old for c in names),
             sum("_" in c for c in names), os.path.join(out, "assigned_clusters.csv")))

    edges, _ = model.edges_from_sketches(ref_db, qry_db, kmers, tbl)
    degree, n_links, links = engine.query_links_dev(edges, refnet.labels_on(edges.device), n_qry, 4)
    print("links: %d queries without a reference within the boundary, %d touching more than one old cluster (at most %d)"
          % (int((degree == 0).sum()), int((n_links > 1).sum()), int(n_links.max())))

    # poppunk_assign --betweenness: every query's betweenness in the network after assignment (the references' edges
    # plus the query-reference edges), highest first; the first lines of the table
    whole = (network._cat([edges, ref_edges]), n_ref + n_qry)
    values = network.vertex_betweenness(whole)[n_ref:]
    print("".join(line + "\n" for line in assign.query_betweenness_table(qNames, values).split("\n")[:6]), end="")
    ref_db.close()
    qry_db.close()


if __name__ == "__main__":
    main()
