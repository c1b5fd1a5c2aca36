"""networkSummary and print_network_summary (PopPUNK/network.py:616-643, 1204-1307) on the MI355X.

    networkSummary(G, calc_betweenness=True, betweenness_sample=100, subsample=None, use_gpu=False)
        -> (metrics [components, density, transitivity, mean betweenness, weighted-mean betweenness],
            scores [base, base (1 - metrics[3]), base (1 - metrics[4])])
    print_network_summary(G, sample_size=None, betweenness_sample=100, use_gpu=False)

follow networkSummary's graph-tool branch: density = E / (0.5 n (n - 1)), transitivity = 3T / W (NaN when W = 0;
unverified against graph-tool, see refine.py), and for every component of more than 3 vertices the maximum of its
exact normalised vertex betweenness (network.py:1288-1294), then their mean and size-weighted mean.  Normalisation is
networkx's betweenness_centrality(normalized=True), sum over sources / ((n_c - 1)(n_c - 2)); that graph-tool's
betweenness(norm=True) gives the same values is UNVERIFIED.

G is an (edges, n_vertices) pair: edges an int64 [m, 2] numpy array or CUDA tensor (each unordered pair once), and
the vertex count; a binding passes (G.get_edges(), G.num_vertices()).  A CUDA tensor is read in place on its device.
`betweenness_sample` and `use_gpu` only steer the reference's cugraph branch: accepted and ignored, unless
`sampled_betweenness=True` asks for that branch's sampled sources (at most betweenness_sample per component, the sample
fixed by `seed`: ppk_network_summary_sampled, this project's sampling rule).  `subsample` (random vertex subsampling)
raises NotImplementedError before the device is touched.  vertex_betweenness(G, norm=True, betweenness_sample=None,
seed=0) is PopPUNK/network.py:1310-1313 on the whole graph.

Cluster numbers: printClusters and printExternalClusters (PopPUNK/network.py:1478-1719).  The
number of every vertex comes from ppk_cluster_sweep / ppk_cluster_sweep_dev (cluster_numbers); the naming rules, the
CSV and the external-cluster table are host code on that number array (name_clusters, print_cluster_numbers), so that
refine.multi_refine hands in the rows of one sweep.

Queries against a loaded network: construct_network_from_assignments and addQueryToNetwork
(PopPUNK/network.py:1115-1203, 1315-1442) on G = (edges, n_vertices[, weights]); query_links and cluster_extend are the
host-array forms of ppk_query_links / ppk_cluster_extend (the CUDA forms are engine.query_links_dev /
engine.cluster_extend_dev), which answer per query what the loaded network matters for: its components.

Minimum spanning trees: generate_minimum_spanning_tree and generate_network_from_distances
(PopPUNK/network.py:1721-1831, 2075-2151) take and return G as (edges, n_vertices, weights); the forest comes from
ppk_mst / ppk_mst_dev and the seed linking (seed_links) runs on the host.

Reference genomes: extractReferences and writeReferences (PopPUNK/network.py:283-509) on G = (edges,
n_vertices); the pick is the deterministic rule of ppk_pick_refs / ppk_pick_refs_dev, not graph-tool's clique order.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib, refine

betweenness_sample_default = refine.betweenness_sample_default


def _counts(G, calc_betweenness, sources=None, seed=0):
    """sources: None = every source (ppk_network_summary); k = at most k per component (ppk_network_summary_sampled)"""
    edges, n = G[:2]
    n = int(n)
    if hasattr(edges, "is_cuda"):
        from . import engine
        if calc_betweenness and sources is not None:
            stats, bt, _, _ = engine.network_summary_sampled_graph_dev(edges, n, sources=sources, seed=seed)
            return stats.cpu().numpy(), bt.cpu().numpy(), n
        if calc_betweenness:
            stats, bt, _, _ = engine.network_summary_graph_dev(edges, n)
            return stats.cpu().numpy(), bt.cpu().numpy(), n
        stats, _ = engine.network_stats_dev(edges, n)
        return stats.cpu().numpy(), None, n
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if calc_betweenness and sources is not None:
        stats, bt, _, _ = refine.network_summary_sampled(e[:, 0], e[:, 1], None, n, 1, sources=sources, seed=seed)
        return stats[0], bt[0], n
    if calc_betweenness:
        stats, bt, _, _ = refine.network_summary(e[:, 0], e[:, 1], None, n, 1)
        return stats[0], bt[0], n
    stats, _ = refine.network_sweep(e[:, 0], e[:, 1], np.zeros(e.shape[0], dtype=np.int64), n, 1)
    return stats[0], None, n


def networkSummary(G, calc_betweenness=True, betweenness_sample=betweenness_sample_default, subsample=None,
                   use_gpu=False, sampled_betweenness=False, seed=0):
    """PopPUNK/network.py:1204-1307, graph-tool branch (see the module docstring).  sampled_betweenness=True: the
    device branch's betweenness_centrality(k=betweenness_sample) instead (network.py:1272-1287): at most
    betweenness_sample sources per component, the sample fixed by `seed` (this project's rule)."""
    if subsample is not None:
        raise NotImplementedError("networkSummary: random vertex subsampling (subsample) is not mirrored")
    if sampled_betweenness and calc_betweenness:
        if int(betweenness_sample) < 1:
            raise ValueError("networkSummary: betweenness_sample must be >= 1")
        stats, bt, n = _counts(G, True, int(betweenness_sample), seed)
    else:
        stats, bt, n = _counts(G, calc_betweenness)
    return refine.summary_from_stats(stats, n, bt)


def vertex_betweenness(G, norm=True, betweenness_sample=None, seed=0):
    """PopPUNK/network.py:1310-1313 on G = (edges, n): float64 numpy [n], every vertex's betweenness in the whole graph,
    networkx's betweenness_centrality(G, normalized=norm): the sum over sources of delta_s(v) over (n - 1)(n - 2) (0
    for every vertex when n <= 2); norm=False gives the pair counts, each unordered pair once.  That graph-tool's
    betweenness(norm=True) normalises the same way is UNVERIFIED.  betweenness_sample = k (this project's addition;
    the reference takes (graph, norm) alone): at most k sources per component under `seed`, scaled by n_c / k
    (ppk_network_summary_sampled).  A CUDA edge tensor is read in place."""
    edges, n = G[:2]
    n = int(n)
    sources = (1 << 31) - 1 if betweenness_sample is None else int(betweenness_sample)
    if sources < 1:
        raise ValueError("vertex_betweenness: betweenness_sample must be >= 1")
    if hasattr(edges, "is_cuda"):
        from . import engine
        values = engine.network_summary_sampled_graph_dev(edges, n, values=True, sources=sources, seed=seed,
                                                          whole_graph=True)[3].cpu().numpy()
    else:
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        values = refine.network_summary_sampled(e[:, 0], e[:, 1], None, n, 1, values_at=0, sources=sources, seed=seed,
                                                whole_graph=True)[3]
    if not norm:
        values = values * (0.5 * float(n - 1) * float(n - 2))
    return values


def print_network_summary(G, sample_size=None, betweenness_sample=betweenness_sample_default, use_gpu=False,
                          sampled_betweenness=False, seed=0):
    """PopPUNK/network.py:616-643: networkSummary's metrics and scores to stderr, in the reference's words."""
    (metrics, scores) = networkSummary(G, subsample=sample_size, betweenness_sample=betweenness_sample,
                                       use_gpu=use_gpu, sampled_betweenness=sampled_betweenness, seed=seed)
    sys.stderr.write("Network summary:\n" + "\n".join(["\tComponents\t\t\t\t" + str(metrics[0]),
                                                       "\tDensity\t\t\t\t\t" + "{:.4f}".format(metrics[1]),
                                                       "\tTransitivity\t\t\t\t" + "{:.4f}".format(metrics[2]),
                                                       "\tMean betweenness\t\t\t" + "{:.4f}".format(metrics[3]),
                                                       "\tWeighted-mean betweenness\t\t" + "{:.4f}".format(metrics[4]),
                                                       "\tScore\t\t\t\t\t" + "{:.4f}".format(scores[0]),
                                                       "\tScore (w/ betweenness)\t\t\t" + "{:.4f}".format(scores[1]),
                                                       "\tScore (w/ weighted-betweenness)\t\t" + "{:.4f}".format(scores[2])])
                     + "\n")


# ---- cluster numbers and names (PopPUNK/network.py:1478-1719) -------------------------------------

def cluster_sweep(i_vec, j_vec, idx_vec, n, n_off=None, device=0):
    """ppk_cluster_sweep on host arrays -> (clusters int32 [n_off, n], n_clusters int32 [n_off]); idx_vec None puts
    every edge at offset 0."""
    i = np.ascontiguousarray(i_vec, dtype=np.int64).ravel()
    j = np.ascontiguousarray(j_vec, dtype=np.int64).ravel()
    o = None if idx_vec is None else np.ascontiguousarray(idx_vec, dtype=np.int64).ravel()
    if i.size != j.size or (o is not None and o.size != i.size):
        raise ValueError("i_vec, j_vec and idx_vec differ in length")
    if n_off is None:
        n_off = int(o.max()) + 1 if o is not None and o.size else 1
    n, n_off = int(n), int(n_off)
    clusters = np.zeros((max(n_off, 1), max(n, 1)), dtype=np.int32)
    counts = np.zeros(max(n_off, 1), dtype=np.int32)
    llp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    rc = _lib.lib().ppk_cluster_sweep(i.ctypes.data_as(llp), j.ctypes.data_as(llp),
                                      o.ctypes.data_as(llp) if o is not None else None, i.size, n, n_off, int(device),
                                      clusters.ctypes.data_as(ip), counts.ctypes.data_as(ip))
    _lib.check(rc, "ppk_cluster_sweep")
    return (clusters if n else clusters[:, :0]), counts


def cluster_numbers(G):
    """printClusters' number (1-based) of every vertex of G = (edges, n_vertices), as an int32 numpy array: components
    in the order of their smallest vertex, ranked by len - rankdata(sizes, 'ordinal') (network.py:1538-1545): by size
    descending, equal sizes by component index descending.  A CUDA edge tensor is read in place."""
    edges, n = G[0], int(G[1])
    if hasattr(edges, "is_cuda"):
        from . import engine
        return engine.cluster_numbers_dev(edges, n)[0].cpu().numpy()
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return cluster_sweep(e[:, 0], e[:, 1], None, n, 1)[0][0]


def clusters_of_numbers(numbers, rlist):
    """newClusters of printClusters from the number array: entry k lists the names of cluster k + 1, in rlist order
    (the reference holds each as a set)."""
    numbers = np.asarray(numbers, dtype=np.int64).ravel()
    if numbers.size != len(rlist):
        raise ValueError("one cluster number per name")
    newClusters = [[] for _ in range(int(numbers.max()) if numbers.size else 0)]
    for name, c in zip(rlist, numbers.tolist()):
        newClusters[c - 1].append(name)
    return newClusters


def name_clusters(newClusters, oldClusters=None):
    """The naming rules of printClusters (network.py:1547-1633) on newClusters (lists of names, in cluster-number
    order) and the old clusters {name: set of samples} in their file order (None: no old file) ->
    (clustering dict, merged_queries list, the set of names the old file knows).

    Without old clusters a cluster's id is its number, an int.  With them ids are str.  A cluster none of whose names
    is known takes the next fresh id, counted on from one above the largest integer that occurs in an old name (the
    parts of a merged name `a_b` included).  Otherwise the old clusters are gone through in file order: one that
    holds ALL of the cluster's known names gives its name and ends the search; each one that holds only some of them
    adds its name to a merged id `a_b...`, and the cluster's unknown names go into merged_queries once per such old
    cluster (as upstream's extend does).  An old cluster met for a second time is reported as split, a merged id as
    merged, both on stderr in the reference's words."""
    if oldClusters is None:
        return ({name: number for number, members in enumerate(newClusters, 1) for name in members}, [], set())
    known = set().union(*oldClusters.values()) if oldClusters else set()
    fresh = 1 + max(int(part) for old_name in oldClusters for part in old_name.split("_"))
    clustering, merged_queries, met = {}, [], set()
    for members in newClusters:
        mine = [name for name in members if name in known]
        unknown = [name for name in members if name not in known]
        if not mine:
            label = str(fresh)
            fresh += 1
        else:
            partial, label = [], None
            for old_name, old_members in oldClusters.items():
                shared = sum(1 for name in mine if name in old_members)
                if shared == 0:
                    continue
                if old_name in met:
                    sys.stderr.write("WARNING: Old cluster %s split across multiple new clusters\n" % old_name)
                met.add(old_name)
                if shared == len(mine):
                    assert not partial, "a cluster matched exactly after a partial match"    # (upstream asserts too)
                    label = old_name
                    break
                partial.append(old_name)
                merged_queries.extend(unknown)
            if label is None:
                label = "_".join(partial)
                sys.stderr.write("Clusters %s have merged into %s\n" % (",".join(label.split("_")), label))
        clustering.update((name, label) for name in members)
    return clustering, merged_queries, known


def write_cluster_csv(clustering, outFileName, oldNames=(), printRef=True):
    """`Taxon,Cluster` rows in blocks of one cluster name each: frequency descending, ties in the order the names were
    first assigned (network.py:1636-1653); inside a block, the order of `clustering` (rlist order within a cluster)."""
    from collections import Counter
    freq_order = sorted(Counter(clustering.values()).items(), key=lambda kv: kv[1], reverse=True)
    position = {name: k for k, (name, _) in enumerate(freq_order)}
    with open(outFileName, 'w') as cluster_file:
        cluster_file.write("Taxon,Cluster\n")
        for cluster_member, cluster_name in sorted(clustering.items(), key=lambda kv: position[kv[1]]):
            if printRef or cluster_member not in oldNames:
                cluster_file.write(",".join((cluster_member, str(cluster_name))) + "\n")


def print_cluster_numbers(numbers, rlist, outPrefix=None, oldClusterFile=None, externalClusterCSV=None, printRef=True,
                          printCSV=True, clustering_type='combined', write_unwords=True):
    """printClusters from the number array of cluster_numbers (or one row of a cluster sweep): everything after the
    component ranking.  See printClusters."""
    from .utils import readIsolateTypeFromCsv
    if oldClusterFile is None and printRef is False:
        raise RuntimeError("Trying to print query clusters with no query sequences")
    if write_unwords and not printCSV:
        write_unwords = False
    newClusters = clusters_of_numbers(numbers, rlist)
    oldClusters = None
    if oldClusterFile is not None:
        oldAllClusters = readIsolateTypeFromCsv(oldClusterFile, mode='external', return_dict=False)
        oldClusters = oldAllClusters[list(oldAllClusters.keys())[0]]
    clustering, merged_queries, oldNames = name_clusters(newClusters, oldClusters)
    if printCSV:
        if write_unwords:
            sys.stderr.write("Pronounceable cluster names are not generated: no _unword_clusters.csv is written\n")
        write_cluster_csv(clustering, outPrefix + "_clusters.csv", oldNames, printRef)
        if externalClusterCSV is not None:
            printExternalClusters(newClusters, externalClusterCSV, outPrefix, oldNames, printRef)
    return clustering, merged_queries


def printClusters(G, rlist, outPrefix=None, oldClusterFile=None, externalClusterCSV=None, printRef=True,
                  printCSV=True, clustering_type='combined', write_unwords=True, use_gpu=False):
    """PopPUNK/network.py:1478-1663, graph-tool branch -> (clustering dict, merged_queries list).

    G = (edges, n_vertices), edges a numpy array or a CUDA tensor read in place; the cluster numbers come from the
    device (cluster_numbers), the rest is print_cluster_numbers.  `<outPrefix>_clusters.csv` holds `Taxon,Cluster`
    and one block per cluster name in the reference's block order; inside a block the reference iterates a Python set,
    so its row order depends on the hash seed -- here the rows of a cluster follow rlist.  Ids are int without an old cluster file and
    str with one.  Unword names need a word list that is not shipped and an unseeded random: `write_unwords` is
    accepted, no `_unword_clusters.csv` is written and one stderr line says so.  `clustering_type` is unused upstream
    too; `use_gpu` selects cugraph upstream (whose value_counts breaks ties differently) and is ignored.
    That graph-tool's label_components numbers components by their lowest vertex is UNVERIFIED."""
    if oldClusterFile is None and printRef is False:
        raise RuntimeError("Trying to print query clusters with no query sequences")
    return print_cluster_numbers(cluster_numbers(G), rlist, outPrefix, oldClusterFile, externalClusterCSV, printRef,
                                 printCSV, clustering_type, write_unwords)


def printExternalClusters(newClusters, extClusterFile, outPrefix, oldNames, printRef=True):
    """PopPUNK/network.py:1665-1719: `<outPrefix>_external_clusters.csv`.  One row per sample (with printRef False only
    those not in oldNames), in cluster order; per external column the labels that any sample of its cluster carries
    there, ';'-joined in sorted order (the reference joins a set), 'NA' when none does.  No row at all: nothing is
    written and the reference's warning goes to stderr."""
    import csv
    from .utils import readIsolateTypeFromCsv
    external = readIsolateTypeFromCsv(extClusterFile, mode='external', return_dict=True)
    table = []
    for members in newClusters:
        cells = []
        for labels_of in external.values():
            seen = sorted({labels_of[sample] for sample in members if sample in labels_of})
            cells.append(";".join(seen) if seen else "NA")
        table.extend([sample] + cells for sample in members if printRef or sample not in oldNames)
    if not table:
        sys.stderr.write("WARNING: No new samples found, cannot write external clusters\n")
        return
    with open(outPrefix + "_external_clusters.csv", 'w', newline='') as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["sample"] + list(external))
        out.writerows(table)


# ---- queries against a loaded network (PopPUNK/network.py:1115-1203, 1315-1442) -----------------

def _assign_arrays(i_vec, j_vec, ref_label):
    i = np.ascontiguousarray(i_vec, dtype=np.int64).ravel()
    j = np.ascontiguousarray(j_vec, dtype=np.int64).ravel()
    if i.size != j.size:
        raise ValueError("i_vec and j_vec differ in length")
    return i, j, np.ascontiguousarray(ref_label, dtype=np.int32).ravel()


def query_links(i_vec, j_vec, ref_label, n_qry, max_links=8, device=0):
    """ppk_query_links on host arrays: vertices 0 .. len(ref_label)-1 are references, the next n_qry the queries;
    ref_label[r] in [0, n_ref) is the component of reference r in the loaded network.  Returns (degree int32 [n_qry]:
    query-reference edges; n_links int32 [n_qry]: distinct labels linked to, exact; links int32 [n_qry, max_links]: the
    smallest max_links of them, ascending, padded with -1).  Edges with both ends on one side are skipped."""
    i, j, lab = _assign_arrays(i_vec, j_vec, ref_label)
    n_qry, max_links = int(n_qry), int(max_links)
    from .engine import check_assign_sizes
    check_assign_sizes("ppk_query_links", lab.size, n_qry, max_links)          # before the outputs are allocated
    degree = np.zeros(max(n_qry, 1), dtype=np.int32)
    n_links = np.zeros(max(n_qry, 1), dtype=np.int32)
    links = np.full((max(n_qry, 1), max_links), -1, dtype=np.int32)
    llp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    rc = _lib.lib().ppk_query_links(i.ctypes.data_as(llp), j.ctypes.data_as(llp), i.size, lab.ctypes.data_as(ip),
                                    lab.size, n_qry, max_links, int(device), degree.ctypes.data_as(ip),
                                    n_links.ctypes.data_as(ip), links.ctypes.data_as(ip))
    _lib.check(rc, "ppk_query_links")
    return degree[:n_qry], n_links[:n_qry], links[:n_qry]


def cluster_extend(i_vec, j_vec, ref_label, n_qry, device=0):
    """ppk_cluster_extend on host arrays -> (numbers int32 [n_ref + n_qry], the cluster count): printClusters' number
    of every vertex of (the loaded network + these edges), the loaded network given by its component labels."""
    i, j, lab = _assign_arrays(i_vec, j_vec, ref_label)
    from .engine import check_assign_sizes
    check_assign_sizes("ppk_cluster_extend", lab.size, int(n_qry))
    n = lab.size + int(n_qry)
    numbers = np.zeros(max(n, 1), dtype=np.int32)
    count = np.zeros(1, dtype=np.int32)
    llp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    rc = _lib.lib().ppk_cluster_extend(i.ctypes.data_as(llp), j.ctypes.data_as(llp), i.size, lab.ctypes.data_as(ip),
                                       lab.size, int(n_qry), int(device), numbers.ctypes.data_as(ip),
                                       count.ctypes.data_as(ip))
    _lib.check(rc, "ppk_cluster_extend")
    return numbers[:n], int(count[0])


def _is_cuda(x):
    return bool(getattr(x, "is_cuda", False))        # (a CPU torch tensor goes the host-array way)


def _cat(parts):
    """the parts one after another, on the device if any of them is there"""
    dev = next((p.device for p in parts if _is_cuda(p)), None)
    if dev is None:
        return np.concatenate([np.asarray(p) for p in parts])
    import torch
    return torch.cat([p if _is_cuda(p) else torch.as_tensor(np.asarray(p), device=dev) for p in parts])


def assignment_edges(assignments, within_label, self_comparison, num_ref, int_offset=0, distMat=None,
                     weights_type=None, weights=None):
    """The new edges of construct_network_from_assignments and their weights (network.py:1170-1184): generateTuples of
    the rows with assignments == within_label, and `weights` filtered to those rows, or process_weights of distMat's.
    A CUDA assignment tensor stays on the device (generate_tuples_dev, edge_weights_dev); numpy arrays go through the
    host-array calls.  Returns (edges int64 [m, 2], weights float32 [m] or None)."""
    from . import poppunk_refine
    if _is_cuda(assignments):
        import torch
        from . import engine
        a = assignments if assignments.dtype == torch.int32 else assignments.to(torch.int32)
        edges = engine.generate_tuples_dev(a.contiguous(), within_label, self_comparison, num_ref, int_offset)
    else:
        assignments = np.asarray(assignments)
        edges = poppunk_refine.generateTuples_array(assignments, within_label, self_comparison, num_ref, int_offset)
    w = None
    if weights is not None:
        w = weights[assignments == within_label]
    elif distMat is not None and weights_type is not None:
        if _is_cuda(distMat):
            import torch
            from . import engine
            e_t = edges if _is_cuda(edges) else torch.as_tensor(edges, device=distMat.device)
            w = engine.edge_weights_dev(distMat, e_t, weights_type, 0 if self_comparison else num_ref, int_offset)
        else:
            a = assignments.cpu().numpy() if _is_cuda(assignments) else assignments
            rows = np.asarray(distMat)[a == within_label, :]
            w = {'euclidean': lambda d: np.linalg.norm(d, axis=1), 'core': lambda d: d[:, 0],
                 'accessory': lambda d: d[:, 1]}[weights_type](rows)
    return edges, w


def _previous_edges(previous_network, vertex_labels, adding_qq_dists, old_ids, previous_pkl, weights):
    """process_previous_network / network_to_edges (network.py:676-732, 519-614) on G = (edges, n[, weights]): the old
    edges under the new numbering, and their weights when `weights`."""
    if previous_pkl is not None:
        raise NotImplementedError("construct_network_from_assignments: previous_pkl (a names pickle) is not "
                                  "mirrored; pass old_ids")
    if old_ids is None:
        sys.stderr.write('Missing .pkl file containing names of sequences in previous network\n')
        sys.exit(1)
    old_edges = previous_network[0]
    old_w = None
    if weights:
        if len(previous_network) < 3 or previous_network[2] is None:
            sys.stderr.write('Loaded network does not have edge weights; try a different '
                             'network or turn off graph weights\n')
            sys.exit(1)
        old_w = previous_network[2]
    if not adding_qq_dists:
        try:
            index = {name: k for k, name in reversed(list(enumerate(vertex_labels)))}      # list.index: the first
            old_id_indices = [index[x] for x in old_ids]
        except KeyError:
            sys.stderr.write("Network size mismatch: a vertex of the previous network is not in the new one\n")
            sys.exit(1)
        if old_id_indices != list(range(len(old_id_indices))):
            remap = np.asarray(old_id_indices, dtype=np.int64)
            if _is_cuda(old_edges):
                import torch
                old_edges = torch.as_tensor(remap, device=old_edges.device)[old_edges]
            else:
                old_edges = remap[np.asarray(old_edges, dtype=np.int64).reshape(-1, 2)]
    return old_edges, old_w


def construct_network_from_assignments(rlist, qlist, assignments, within_label=1, int_offset=0, weights=None,
                                       distMat=None, weights_type=None, previous_network=None, old_ids=None,
                                       adding_qq_dists=False, previous_pkl=None,
                                       betweenness_sample=betweenness_sample_default, summarise=True, sample_size=None,
                                       use_gpu=False):
    """PopPUNK/network.py:1115-1203 with the reference's signature, on G = (edges, n_vertices), or (edges, n_vertices,
    weights) when weights are asked for (`weights`, or distMat with weights_type).  The new edges come first, in
    generateTuples' order, then the previous network's (construct_network_from_edge_list, network.py:822-834).
    `assignments` (and distMat) may be numpy arrays or CUDA tensors; a CUDA assignment gives CUDA edges.
    previous_network is such a G, its vertices named by old_ids; the reference's messages and exits are kept for a
    previous network without weights when weights are asked for and for old names missing from the new list.
    previous_pkl raises NotImplementedError (file loading is not mirrored); `use_gpu` is accepted and ignored."""
    rlist, qlist = list(rlist), list(qlist)
    self_comparison = rlist == qlist
    vertex_labels = rlist if self_comparison else rlist + qlist
    edges, w = assignment_edges(assignments, within_label, self_comparison, len(rlist), int_offset, distMat,
                                weights_type, weights)
    if previous_network is not None:
        old_edges, old_w = _previous_edges(previous_network, vertex_labels, adding_qq_dists, old_ids, previous_pkl,
                                           w is not None)
        old_edges = old_edges if _is_cuda(old_edges) else np.asarray(old_edges, dtype=np.int64).reshape(-1, 2)
        edges = _cat([edges, old_edges])
        if w is not None:
            w = _cat([w if _is_cuda(w) else np.asarray(w, dtype=np.float32),
                      old_w if _is_cuda(old_w) else np.asarray(old_w, dtype=np.float32)])
    G = (edges, len(vertex_labels)) if w is None else (edges, len(vertex_labels), w)
    if summarise:
        print_network_summary(G[:2], sample_size=sample_size, betweenness_sample=betweenness_sample, use_gpu=use_gpu)
    return G


def model_assign(model, X, slope=None):
    """model.assign(X[, slope=slope]) as upstream calls it; a CUDA matrix goes to the model's assign_dev"""
    fn = model.assign_dev if _is_cuda(X) else model.assign
    return fn(X) if slope is None else fn(X, slope=slope)


def query_degrees(edges, n_ref, n_qry):
    """G.get_total_degrees of the query vertices (network.py:1395) from the query-reference edges alone (the previous
    network has no edge at a query): the degree array of query_links under labels that do not matter (all zero)."""
    if _is_cuda(edges):
        import torch
        from . import engine
        lab = torch.zeros(n_ref, dtype=torch.int32, device=edges.device)
        return engine.query_links_dev(edges.contiguous(), lab, n_qry, 1)[0].cpu().numpy()
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return query_links(e[:, 0], e[:, 1], np.zeros(n_ref, dtype=np.int32), n_qry, 1)[0]


def addQueryToNetwork(dbFuncs, rList, qList, G, assignments, model, queryDB, kmers=None, distance_type='euclidean',
                      queryQuery=False, strand_preserved=False, weights=None, threads=1, use_gpu=False):
    """PopPUNK/network.py:1315-1442 with the reference's signature -> (G, qqDistMat), G = (edges, n[, weights]).

    The query-reference edges of `assignments` are put in front of G's; a query left without an edge switches on the
    query-query distances, as upstream ("Found novel query clusters..."), which come from dbFuncs['queryDatabase']
    (called with the reference's keywords; a CUDA tensor it returns stays on the device), are assigned by `model` under distance_type's slope and added in front
    again.  One query never needs them (an empty [0, 2] matrix is returned); more than one without `kmers` is the
    reference's RuntimeError.  `weights` is the query-reference distance matrix, as upstream passes it; G must then
    carry weights too (the reference's message and exit otherwise).  addRandom (network.py:1408) is NOT called:
    sketching and the random-match table of the query database are out of scope, queryDatabase is expected to find
    them.  `use_gpu` is accepted and ignored."""
    queryDatabase = dbFuncs['queryDatabase']
    if len(qList) > 1 and kmers is None:
        raise RuntimeError("Must provide db querying info (kmers) if adding "
                           "more than one sample, as q-q dists may be needed")
    weights_type = None if weights is None else distance_type
    qqDistMat = None
    ref_count = len(rList)
    n_old = int(G[0].shape[0]) if hasattr(G[0], "shape") else len(G[0])
    G = construct_network_from_assignments(rList, qList, assignments, within_label=model.within_label,
                                           previous_network=G, old_ids=rList, distMat=weights,
                                           weights_type=weights_type, summarise=False, use_gpu=use_gpu)
    if not queryQuery:
        # the new edges are in front of the previous network's, which has none at a query and is not read again
        edge_count = query_degrees(G[0][:G[0].shape[0] - n_old], ref_count, len(qList))
        if np.any(edge_count == 0):
            sys.stderr.write("Found novel query clusters. Calculating distances between them.\n")
            queryQuery = True
    if queryQuery:
        if len(qList) == 1:
            qqDistMat = np.zeros((0, 2), dtype=np.float32)
        else:
            sys.stderr.write("Calculating all query-query distances\n")
            qqDistMat = queryDatabase(rNames=qList, qNames=qList, dbPrefix=queryDB, queryPrefix=queryDB, klist=kmers,
                                      self=True, number_plot_fits=0, threads=threads)
            if distance_type == 'core':
                queryAssignation = model_assign(model, qqDistMat, 0)
            elif distance_type == 'accessory':
                queryAssignation = model_assign(model, qqDistMat, 1)
            else:
                queryAssignation = model_assign(model, qqDistMat)
            vertex_labels = list(rList) + list(qList)
            G = construct_network_from_assignments(vertex_labels, vertex_labels, queryAssignation,
                                                   int_offset=ref_count, within_label=model.within_label,
                                                   previous_network=G, old_ids=vertex_labels, adding_qq_dists=True,
                                                   distMat=qqDistMat, weights_type=weights_type, summarise=False,
                                                   use_gpu=use_gpu)
    return G, qqDistMat


# ---- minimum spanning trees (PopPUNK/network.py:1721-1831, 2075-2151) ----------------------------

def kruskal(edges, n, weights):
    """A plain host Kruskal under the device's total order (w, min(i, j), max(i, j), index): the input indices of the
    minimum spanning forest, ascending.  The MST callable of seed_links on the host (tests, small graphs)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(weights, dtype=np.float64).ravel() + 0.0      # -0.0 -> +0.0
    lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    order = np.lexsort((np.arange(e.shape[0]), hi, lo, w))
    parent = list(range(int(n)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    keep = []
    for k in order.tolist():
        a, b = find(int(e[k, 0])), find(int(e[k, 1]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            keep.append(k)
    return np.array(sorted(keep), dtype=np.int64)


def device_mst(edges, n, weights, device=0):
    """ppk_mst on host arrays (weights as float32) -> the input indices of the forest, ascending."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    i, j = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if w.size != i.size:
        raise ValueError("one weight per edge")
    tree = np.zeros(max(min(i.size, int(n) - 1), 1), dtype=np.int64)
    n_tree = C.c_ulonglong(0)
    llp = C.POINTER(C.c_longlong)
    rc = _lib.lib().ppk_mst(i.ctypes.data_as(llp), j.ctypes.data_as(llp), w.ctypes.data_as(C.POINTER(C.c_float)),
                            i.size, int(n), int(device), tree.ctypes.data_as(llp), C.byref(n_tree), None)
    _lib.check(rc, "ppk_mst")
    return tree[:n_tree.value]


def forest_seeds(forest_edges, n):
    """The seed of every component of a forest as generate_minimum_spanning_tree picks it (network.py:1773-1781):
    components numbered as label_components numbers them (by smallest vertex), and in each the first vertex, in vertex
    order, of maximum degree within the forest.  Returns (seeds as the reference's set, iterated in its order; the
    number of components)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(forest_edges, dtype=np.int64).reshape(-1, 2)
    n = int(n)
    adj = coo_matrix((np.ones(f.shape[0]), (f[:, 0], f[:, 1])), shape=(n, n))
    n_comp, labels = connected_components(adj, directed=False)
    seed_vertices = set()
    if n_comp > 1:
        degree = np.bincount(f.ravel(), minlength=n)
        order = np.lexsort((-degree, labels))             # by component, then degree descending, then vertex (stable)
        first = np.ones(n, dtype=bool)
        first[1:] = labels[order][1:] != labels[order][:-1]
        for v in order[first].tolist():                    # component order, as the reference's loop
            seed_vertices.add(v)
    return seed_vertices, n_comp


def link_seeds(seed_vertices, g_edges, g_weights, max_weight, mst):
    """The reference's seed graph and its MST (network.py:1799-1829): for each seed in set order, every edge of G at
    that seed whose other end is a seed (orientation: the seed first); a seed with none connects to every other seed at
    max_weight.  `g_edges` / `g_weights` may be just G's edges between two seeds, in G's order.  Returns the seed MST's
    edges int64 [k, 2] and weights float64 [k] in the seed graph's edge order."""
    seeds = list(seed_vertices)
    is_seed = set(seeds)
    g = np.asarray(g_edges, dtype=np.int64).reshape(-1, 2)
    gw = np.asarray(g_weights, dtype=np.float64).ravel()
    both = np.isin(g[:, 0], seeds) & np.isin(g[:, 1], seeds)
    g, gw = g[both], gw[both]
    parts, wparts = [], []
    s_arr = np.array(seeds, dtype=np.int64)
    for ref in seeds:
        at0, at1 = g[:, 0] == ref, g[:, 1] == ref
        hit = np.flatnonzero(at0 | at1)                     # G's edges at ref, in G's order
        other = np.where(at0[hit], g[hit, 1], g[hit, 0])
        if hit.size and all(int(o) in is_seed for o in other):
            parts.append(np.stack([np.full(hit.size, ref), other], axis=1))
            wparts.append(gw[hit])
        else:
            q = s_arr[s_arr != ref]
            parts.append(np.stack([np.full(q.size, ref), q], axis=1))
            wparts.append(np.full(q.size, float(max_weight)))
    conn = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int64)
    cw = np.concatenate(wparts) if wparts else np.zeros(0)
    n_seed_g = int(conn.max()) + 1 if conn.size else 0
    keep = np.sort(np.asarray(mst(conn, n_seed_g, cw), dtype=np.int64))
    return conn[keep], cw[keep]


def seed_links(forest_edges, g_edges, g_weights, n, mst):
    """The host step of generate_minimum_spanning_tree after the forest (network.py:1771-1829), a pure function of
    (the forest's edges, G's edges and weights, n, an MST callable mst(edges, n, weights) -> indices).  Returns the
    edges int64 [k, 2] and weights float64 [k] it appends to the forest (none for a connected forest).  See
    generate_minimum_spanning_tree for the quirks it keeps."""
    seeds, n_comp = forest_seeds(forest_edges, n)
    if n_comp <= 1:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    gw = np.asarray(g_weights, dtype=np.float64).ravel()
    max_weight = float(np.max(gw))                            # ValueError without edges, as np.max upstream
    return link_seeds(seeds, g_edges, gw, max_weight, mst)


def generate_minimum_spanning_tree(G, from_cugraph=False):
    """PopPUNK/network.py:1721-1831, graph-tool branch, with the forest from the device (ppk_mst / ppk_mst_dev).

    G = (edges, n_vertices, weights): edges int64 [m, 2] and weights [m] as numpy arrays or CUDA tensors (int64 /
    float32, read in place on their device), parallel edges allowed.  Returns the same triple as numpy arrays: the
    forest's edges in G's edge order (gt.Graph(GraphView(G, efilt=mst), prune=True) keeps that order) followed by the
    seed MST's edges, and their weights.  `from_cugraph` is accepted and ignored (this is the device path either way).

    Reproduced as the reference has them:
      - the forest is the unique one under (w, min, max, index); among equal weights the reference's choice is boost
        Kruskal's and implementation-defined.  Weights are read as float32.
      - seeds: per forest component (numbered by smallest vertex), the first vertex in vertex order of maximum degree
        in the forest; they are kept in a Python set and the seed graph is built in that set's iteration order.
      - the forest spans G's components, so G has no edge between two seeds: every seed takes the fallback and
        connects to every other seed at max_weight = max of G's weights, each pair in both orientations.  The branch
        that takes G's own seed-to-seed edges is kept (seed_links reaches it with any forest).
      - the seed MST is taken over that graph as it stands; a seed graph that stays disconnected (possible only in
        the seed-to-seed branch) leaves the result disconnected.
      - the seed MST's edges are appended with add_edge_list and no edge property, so their weight in the returned
        graph is 0.0 (graph-tool initialises a new edge's property value; unverified, graph-tool is not available).
      - G without edges and more than one vertex: np.max of no weights raises ValueError.
    """
    edges, n, weights = G
    n = int(n)
    if hasattr(edges, "is_cuda"):
        from . import engine
        import torch
        w_t = weights if hasattr(weights, "is_cuda") else torch.as_tensor(
            np.asarray(weights, dtype=np.float32), device=edges.device)
        tree, n_comp, _ = engine.mst_dev(edges, w_t, n)
        forest = edges[tree].cpu().numpy()
        forest_w = w_t[tree].double().cpu().numpy()
        if n_comp > 1:
            seeds, _ = forest_seeds(forest, n)
            s = torch.zeros(max(n, 1), dtype=torch.bool, device=edges.device)
            s[torch.as_tensor(sorted(seeds), dtype=torch.int64, device=edges.device)] = True
            both = s[edges[:, 0]] & s[edges[:, 1]]
            max_weight = float(w_t.max().item())              # RuntimeError without edges (upstream: ValueError)
            add, _ = link_seeds(seeds, edges[both].cpu().numpy(), w_t[both].double().cpu().numpy(), max_weight,
                                lambda e, k, w: engine.mst_dev(torch.as_tensor(e, device=edges.device),
                                                               torch.as_tensor(w, dtype=torch.float32,
                                                                               device=edges.device), k)[0].cpu().numpy())
        else:
            add = np.zeros((0, 2), dtype=np.int64)
    else:
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        w = np.asarray(weights, dtype=np.float32).ravel()
        tree = device_mst(e, n, w)
        forest, forest_w = e[tree], w[tree].astype(np.float64)
        add, _ = seed_links(forest, e, w, n, device_mst)
    out_e = np.concatenate([forest, add.astype(np.int64)]) if add.size else forest
    out_w = np.concatenate([forest_w, np.zeros(add.shape[0])])     # the appended edges' weight: 0.0
    return out_e, n, out_w


def generate_network_from_distances(mode, model, core_distMat=None, acc_distMat=None, sparse_mat=None,
                                    previous_mst=None, combined_seq=None, rlist=None, old_rlist=None,
                                    distance_type='core', threads=1, gpu_graph=False):
    """PopPUNK/network.py:2075-2151 with the reference's signature; returns G as (edges, n, weights).

    dense: the model's device assignment of every row of the [n_pairs, 2] distance matrix, generate_tuples_dev of the
    within label (a self network over combined_seq) and edge_weights_dev of `distance_type` -- the weighted network
    that the caller passes to generate_minimum_spanning_tree, as upstream (CUDA tensors).  core_distMat may be that
    resident float32 [n_pairs, 2] CUDA tensor itself (acc_distMat None), or core_distMat / acc_distMat the square numpy
    matrices of upstream (squareToLong on the host, then uploaded).
    sparse: generate_mst_from_sparse_input (poppunk_amd.sparse_mst): the MST of a kNN graph.
    `previous_mst` (not None) raises NotImplementedError: merging needs name remapping through network_to_edges.
    `threads` and `gpu_graph` are accepted and ignored."""
    if previous_mst is not None:
        raise NotImplementedError("generate_network_from_distances: previous_mst merging is not mirrored")
    if mode == 'sparse':
        from . import sparse_mst
        return sparse_mst.generate_mst_from_sparse_input(sparse_mat, rlist, old_rlist=old_rlist,
                                                         previous_mst=previous_mst, gpu_graph=gpu_graph)
    if mode != 'dense':
        sys.stderr.write('Unknown network mode - expect dense or sparse\n')
        return None
    import torch
    from . import engine, pp_sketchlib
    if hasattr(core_distMat, "is_cuda") and acc_distMat is None:
        dist_t = core_distMat
    else:
        dist = np.hstack((pp_sketchlib.squareToLong(core_distMat, threads).reshape(-1, 1),
                          pp_sketchlib.squareToLong(acc_distMat, threads).reshape(-1, 1))).astype(np.float32)
        dist_t = torch.as_tensor(np.ascontiguousarray(dist), device="cuda")
    assign = model.assign_dev(dist_t)
    if assign.dtype != torch.int32:
        assign = assign.to(torch.int32)
    edges = engine.generate_tuples_dev(assign.contiguous(), model.within_label)
    w = engine.edge_weights_dev(dist_t, edges, distance_type)
    n = len(combined_seq) if combined_seq is not None else engine._samples_of(dist_t.shape[0])
    return edges, n, w


# ---- reference genomes (PopPUNK/network.py:283-509) ------------------------------------------------

def _pick_references(edges, n, existing, merged, fast):
    """the engine call of extractReferences: (is_ref, ref_edges, counts), on the device of a CUDA edge tensor"""
    from . import engine
    if _is_cuda(edges):
        import torch
        up = [None if f is None else torch.as_tensor(f, device=edges.device) for f in (existing, merged)]
        return engine.pick_references_dev(edges, n, up[0], up[1], fast)
    return engine.pick_references(edges, n, existing, merged, fast)


def _name_flags(names, dbOrder, what):
    """uint8 [len(dbOrder)]: 1 where the name is listed; an unknown name is a KeyError, as upstream's index_lookup"""
    index_lookup = {v: k for k, v in enumerate(dbOrder)}
    flags = np.zeros(len(dbOrder), dtype=np.uint8)
    for r in frozenset(names):
        if r not in index_lookup:
            raise KeyError("%s %r is not in dbOrder" % (what, r))
        flags[index_lookup[r]] = 1
    return flags


def extractReferences(G, dbOrder, outPrefix, merged_queries=list(), outSuffix='', existingRefs=None, threads=1,
                      use_gpu=False, fast_mode=False):
    """PopPUNK/network.py:283-487 with the reference's argument order, stderr lines and return order
    (reference_indices, reference_names, refFileName, G_ref), by the deterministic rule of DESIGN.md 3.25
    (ppk_pick_refs / ppk_pick_refs_dev) in place of graph-tool's clique enumeration: which genomes are picked differs
    from upstream, what the pick guarantees does not.

    G is the (edges, n_vertices) pair of this module (a CUDA edge tensor is read in place) and G_ref such a pair over
    the references, vertex k being the k-th reference in dbOrder.  reference_indices is a SORTED int64 array where the
    reference returns a set.  `threads` and `use_gpu` are accepted and ignored; the cugraph Leiden branch is not
    mirrored."""
    edges, n = G[0], int(G[1])
    if n != len(dbOrder):
        raise ValueError("one name in dbOrder per vertex of G")
    existing = None if existingRefs is None else _name_flags(existingRefs, dbOrder, "existing reference")
    merged = _name_flags(merged_queries, dbOrder, "merged query") if len(merged_queries) > 0 else None
    sys.stderr.write("Running quick reference picking\n" if fast_mode else "Running clique finding\n")
    is_ref, ref_edges, counts = _pick_references(edges, n, existing, merged, bool(fast_mode))
    sys.stderr.write("Reconstructing clusters with shortest paths\n")
    flags = is_ref.cpu().numpy() if hasattr(is_ref, "cpu") else np.asarray(is_ref)
    reference_indices = np.flatnonzero(flags).astype(np.int64)
    reference_names = [dbOrder[int(x)] for x in reference_indices]
    refFileName = writeReferences(reference_names, outPrefix, outSuffix=outSuffix)
    return reference_indices, reference_names, refFileName, (ref_edges, len(reference_names))


def writeReferences(refList, outPrefix, outSuffix=""):
    """PopPUNK/network.py:489-509: the names, one a line, to <outPrefix>/<basename(outPrefix)><outSuffix>.refs; returns
    the file's name."""
    name = "%s/%s%s.refs" % (outPrefix, os.path.basename(outPrefix), outSuffix)
    with open(name, "w") as f:
        f.write("".join(ref + "\n" for ref in refList))
    return name
