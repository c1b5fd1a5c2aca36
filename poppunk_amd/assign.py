"""poppunk_assign's last step on the MI355X: from query-reference distances, or straight from
sketches, to a cluster name per query -- the part of assign_query_hdf5 after the network is loaded
(PopPUNK/assign.py:575-733), with network.addQueryToNetwork (network.py:1315-1442) and qc.qcQueryAssignments
(qc.py:372-417).

For assignment the reference network matters only through its components: two references are in one cluster of
(network + new edges) iff a chain of new edges joins their components.  ReferenceNetwork therefore computes the
component label of every reference once and keeps it on the device; no call here reads the network's edges again.

    refnet = ReferenceNetwork(G, rNames, old_cluster_file)
    res = assign_query_clusters(dbFuncs, refnet, qNames, qrDistMat, model, output, kmers=kmers)     # from distances
    res = assign_from_sketches(ref_db, qry_db, model, refnet, qNames, kmers, random_tbl, output)    # matrix never formed

EXACTNESS CONDITION: the labels must be the components of the network the reference would have loaded.  Then every
mode gives the reference's result on that network; with other labels it gives the reference's result on a network that
has those components.

Device results and host naming are kept apart, as cluster_numbers / print_cluster_numbers are: the device gives number
and link arrays (query_links, cluster_extend), the names come from network.name_clusters on lists.

Not mirrored: --update-db and database joining (extractReferences itself is
network.extractReferences); the lineage branch here (it
is lineages.extend_strain_lineages, DESIGN.md 3.22: every strain's LineageFit.extend in one pass); fetchNetwork's file
loading (G arrives loaded); `stable` without a distance matrix; printExternalClusters under `serial` / `stable` (upstream
hands it a dict where it expects lists of names).  No _unword_clusters.csv is written (network.printClusters).
"""
import os
import sys
from operator import itemgetter

import numpy as np

from . import network, qc
from .utils import readIsolateTypeFromCsv

MAX_LINKS = 64          # ppk_query_links' widest row; a query linked to more components is finished on the host


_is_cuda = network._is_cuda


def component_labels(G):
    """int32 [n] CUDA: every vertex's component in G = (edges, n), numbered in the order of the components' lowest
    vertices (network_stats_dev(labels=True)).  Numpy edges are uploaded."""
    import torch
    from . import engine
    edges = G[0]
    if not _is_cuda(edges):
        edges = torch.as_tensor(np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2)), device="cuda")
    return engine.network_stats_dev(edges.contiguous(), int(G[1]), labels=True)[1]


class ReferenceNetwork:
    """The loaded reference network as assignment needs it: G = (edges, n[, weights]), the reference names in vertex
    order, the old cluster file, and the component label of every reference -- computed once (component_labels) and kept
    on the device (`labels_t`; `labels` is the host copy, fetched on first use).  `labels` may be passed instead (an
    int array with values in [0, n), e.g. from a saved clustering): see the exactness condition in the module
    docstring.  A vertex count that differs from len(rNames) is the reference's error and exit (assign.py:586-590)."""

    def __init__(self, G, rNames, old_cluster_file, labels=None):
        self.G, self.rNames, self.old_cluster_file = G, list(rNames), old_cluster_file
        n_vertices = int(G[1])
        if n_vertices != len(self.rNames):
            sys.stderr.write(f"ERROR: There are {n_vertices} vertices in the network but {len(self.rNames)} reference "
                             "names supplied; please check the '--model-dir' variable is pointing to the correct "
                             "directory\n")
            sys.exit(1)
        self._labels = self.labels_t = None
        if labels is None:
            labels = component_labels(G)
        if _is_cuda(labels):
            self.labels_t = labels
        else:
            self._labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()

    @property
    def labels(self):
        if self._labels is None:
            self._labels = self.labels_t.cpu().numpy()
        return self._labels

    def labels_on(self, device):
        if self.labels_t is None or self.labels_t.device != device:
            import torch
            self.labels_t = torch.as_tensor(self.labels, device=device)
        return self.labels_t


# ---- the two device results, for edges on either side -----------------------------------------------------------
def links_of(edges, refnet, n_qry, max_links):
    """(degree, n_links, links) numpy arrays of query_links for a numpy or CUDA edge list"""
    if _is_cuda(edges):
        from . import engine
        return tuple(t.cpu().numpy() for t in engine.query_links_dev(edges.contiguous(), refnet.labels_on(edges.device),
                                                                     n_qry, max_links))
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return network.query_links(e[:, 0], e[:, 1], refnet.labels, n_qry, max_links)


def extend_numbers(edges, refnet, n_qry):
    """cluster numbers (numpy int32 [n_ref + n_qry]) of (the loaded network + edges) for a numpy or CUDA edge list"""
    if _is_cuda(edges):
        from . import engine
        return engine.cluster_extend_dev(edges.contiguous(), refnet.labels_on(edges.device), n_qry)[0].cpu().numpy()
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return network.cluster_extend(e[:, 0], e[:, 1], refnet.labels, n_qry)[0]


def nearest_reference(qrDistMat, n_qry, n_ref, dist_col):
    """the reference index of every query's kNN = 1 neighbour (engine.nearest_reference_dev), as a numpy array; a
    numpy matrix is uploaded"""
    import torch
    from . import engine
    d = qrDistMat if _is_cuda(qrDistMat) else torch.as_tensor(
        np.ascontiguousarray(qrDistMat, dtype=np.float32), device="cuda")
    return engine.nearest_reference_dev(d.contiguous(), n_qry, n_ref, dist_col).cpu().numpy()


# ---- host naming ---------------------------------------------------------------------------------------------------
def old_clusters_of(old_cluster_file):
    """the old clusters {name: set of samples} in file order, as printClusters reads them (network.py:1530-1532)"""
    oldAllClusters = readIsolateTypeFromCsv(old_cluster_file, mode='external', return_dict=False)
    return oldAllClusters[list(oldAllClusters.keys())[0]]


def linked_labels(q, n_links, links, edges, ref_labels, n_ref):
    """the distinct labels query q is linked to: its row of `links`, or, when the row is too narrow, from its edges"""
    if n_links[q] <= links.shape[1]:
        return links[q, :n_links[q]].tolist()
    e = edges.cpu().numpy() if _is_cuda(edges) else np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    lo, hi = e.min(axis=1), e.max(axis=1)
    return np.unique(ref_labels[lo[(hi == n_ref + q) & (lo < n_ref)]]).tolist()


def serial_names(rNames, qNames, degree, n_links, links, edges, ref_labels, oldClusters):
    """The loop of assign.py:696-722 from one query_links result: every query alone against the loaded network.  The
    reference copies the graph, adds the query's edges and runs printClusters on all of it; the query's name depends
    only on the cluster it lands in -- {the references of its linked components, the query} -- so name_clusters is
    run on that one cluster.  Kept as upstream has it: int() of the name, and `> len(rNames)` -> "novel" (a fresh id
    that is not larger stays an int).  int() of a merged name `a_b` is whatever Python makes of it: since Python 3.6
    the underscore is a digit separator and '5_4' reads as 54 (so usually "novel"); a name int() rejects raises
    ValueError, after its "have merged" line, as it does upstream.
    Every reference must be in the old cluster file (then no other cluster of the network is renamed or reported and
    the fresh id does not depend on the others): NotImplementedError naming the first that is not."""
    known = set().union(*oldClusters.values()) if oldClusters else set()
    for name in rNames:
        if name not in known:
            raise NotImplementedError("serial assignment: reference %s is not in the old cluster file" % name)
    members_of = {}
    for name, lab in zip(rNames, np.asarray(ref_labels).tolist()):
        members_of.setdefault(lab, []).append(name)
    isolateClustering = {}
    for idx, sample in enumerate(qNames):
        if degree[idx] == 0:
            sys.stderr.write("Found novel query clusters. Calculating distances between them.\n")
        members = [name for lab in linked_labels(idx, n_links, links, edges, np.asarray(ref_labels), len(rNames))
                   for name in members_of[lab]]
        isolate_cluster = network.name_clusters([members + [sample]], oldClusters)[0]
        cluster = int(isolate_cluster[sample])
        if cluster > len(rNames):
            cluster = "novel"
        isolateClustering[sample] = cluster
    return isolateClustering


def stable_names(rNames, qNames, ref_idxs, linked, refClustering):
    """assign.py:685-691: a query takes its nearest reference's cluster when that distance was assigned within-strain
    (linked[q]), "NA" otherwise"""
    return {qNames[q]: (refClustering[rNames[ref]] if is_in else "NA")
            for q, (ref, is_in) in enumerate(zip(np.asarray(ref_idxs).tolist(), np.asarray(linked).tolist()))}


def write_query_csv(isolateClustering, output):
    """assign.py:724-729"""
    with open(f"{output}/{os.path.basename(output)}_clusters.csv", 'w') as cluster_f:
        cluster_f.write("Taxon,Cluster\n")
        for sample, cluster in isolateClustering.items():
            cluster_f.write(",".join((sample, str(cluster))) + "\n")


def _prune(rNames, qNames, failed, qrDistMat, queryAssignments):
    if not _is_cuda(qrDistMat) and not _is_cuda(queryAssignments):
        return qc.prune_query_distance_matrix(rNames, qNames, failed, qrDistMat, queryAssignments)
    import torch
    keep = [q for q, name in enumerate(qNames) if name not in failed]

    def rows(x):
        if not _is_cuda(x):
            return qc.prune_query_distance_matrix(rNames, qNames, failed, x)[1]
        k = torch.as_tensor(keep, dtype=torch.int64, device=x.device)
        return x.reshape((len(qNames), len(rNames)) + tuple(x.shape[1:]))[k].reshape((-1,) + tuple(x.shape[1:]))
    return [qNames[q] for q in keep], rows(qrDistMat), rows(queryAssignments)


def query_betweenness_table(qNames, betweenness):
    """The text of poppunk_assign --betweenness (PopPUNK/assign.py:648-651): the header, then one line per query, by
    descending betweenness, equal values in the queries' order (Python's stable sort, as the reference's)."""
    query_betweenness = {query: b for query, b in zip(qNames, betweenness)}
    lines = ["query\tbetweenness"]
    for query, q_betweenness in sorted(query_betweenness.items(), key=itemgetter(1), reverse=True):
        lines.append(f"{query}\t{q_betweenness}")
    return "\n".join(lines) + "\n"


def assign_query_clusters(dbFuncs, refnet, qNames, qrDistMat, model, output, kmers=None, fit_type='default',
                          qc_dict=None, graph_weights=False, serial=False, stable=None, update_db=False,
                          write_references=False, external_clustering=None, strand_preserved=False, threads=1,
                          file_extension_string='', gpu_graph=False, return_network=False):
    """The body of assign_query_hdf5 at PopPUNK/assign.py:592-733 on loaded pieces: refnet (a ReferenceNetwork), the
    query names, qrDistMat float32 [n_qry * n_ref, 2] (numpy, or a CUDA tensor, which keeps every array on the
    device) and the fitted model.  Returns a dict: isolateClustering (joint mode: {'combined': {name: cluster}}, as
    upstream; serial / stable: {query: cluster}), merged_queries (joint mode, else None), qNames (after QC),
    qqDistMat, genomeNetwork (joint mode with return_network=True: the new edges in front of the loaded network's,
    else None).

      joint  (default)   the query-reference edges, query-query edges when a query is unlinked (addQueryToNetwork's
                         rule and messages), ONE cluster_extend over the new edges, then print_cluster_numbers
      serial=True        one query_links call for all queries, then serial_names; writes <output>/<output>_clusters.csv
      stable='core' / 'accessory' (with serial=True, as upstream nests it)   the kNN = 1 call on the matrix plus a
                         gather of the assignment (stable_names); matrix route only

    qc_dict {'run_qc', 'max_merge', 'betweenness'}: with run_qc and max_merge > 1, qcQueryAssignments and the
    reference's report, exit when every query fails, and pruning; with run_qc and 'betweenness' (joint mode), the
    table of every query's betweenness in the whole network after assignment goes to stdout (assign.py:646-651,
    network.vertex_betweenness; this is the one step that reads the loaded network's edges); 'betweenness_sample'
    (absent: every source) and 'betweenness_seed' are this project's additions.
    graph_weights needs a loaded network with weights (the reference's message and exit otherwise).
    update_db only widens printRef, as upstream's `write_references or update_db`; nothing is updated."""
    rNames, qNames = refnet.rNames, list(qNames)
    old_cluster_file = refnet.old_cluster_file
    qc_dict = qc_dict or {'run_qc': False}

    # Assign these distances as within or between strain
    if fit_type == 'core_refined' or (getattr(model, 'type', None) == 'refine' and getattr(model, 'threshold', False)):
        queryAssignments = network.model_assign(model, qrDistMat, 0)
        dist_type = 'core'
    elif fit_type == 'accessory_refined':
        queryAssignments = network.model_assign(model, qrDistMat, 1)
        dist_type = 'accessory'
    else:
        queryAssignments = network.model_assign(model, qrDistMat)
        dist_type = 'euclidean'

    # QC assignments to check for multi-links
    if qc_dict['run_qc'] and qc_dict.get('max_merge', 0) > 1:
        sys.stderr.write("Running QC on model assignments\n")
        seq_names_passing = frozenset(qc.qcQueryAssignments(rNames, qNames, queryAssignments, qc_dict['max_merge'],
                                                            old_cluster_file)[0])
        failed_samples = [name for name in qNames if name not in seq_names_passing]      # (upstream: a frozenset)
        if len(failed_samples) > 0:
            sys.stderr.write(f"{len(failed_samples)} samples failed:\n"
                             f"{','.join(failed_samples)}\n")
            if len(failed_samples) == len(qNames):
                sys.exit(1)
            qNames, qrDistMat, queryAssignments = _prune(rNames, qNames, frozenset(failed_samples), qrDistMat,
                                                         queryAssignments)

    weights = qrDistMat if graph_weights else None
    output_fn = os.path.join(output, os.path.basename(output) + file_extension_string)
    result = {"isolateClustering": None, "merged_queries": None, "qNames": qNames, "qqDistMat": None,
              "genomeNetwork": None}
    n_ref, n_qry = len(rNames), len(qNames)
    if not serial:
        # the new edges alone: addQueryToNetwork on a network of the loaded one's vertices and no edges
        loaded = refnet.G
        none = (np.zeros((0, 2), dtype=np.int64), n_ref) + \
            ((np.zeros(0, dtype=np.float32),) if len(loaded) > 2 and loaded[2] is not None else ())
        new, qqDistMat = network.addQueryToNetwork(dbFuncs, rNames, qNames, none, queryAssignments, model, output,
                                                   kmers=kmers, distance_type=dist_type,
                                                   queryQuery=update_db and fit_type == 'default',
                                                   strand_preserved=strand_preserved, weights=weights,
                                                   threads=threads, use_gpu=gpu_graph)
        if qc_dict['run_qc'] and qc_dict.get('betweenness'):
            # assign.py:646-651: every query's betweenness in the whole network after assignment
            whole = (network._cat([new[0], loaded[0]]), n_ref + n_qry)
            values = network.vertex_betweenness(whole, betweenness_sample=qc_dict.get('betweenness_sample'),
                                                seed=qc_dict.get('betweenness_seed', 0))
            sys.stdout.write(query_betweenness_table(qNames, values[n_ref:n_ref + n_qry]))
        numbers = extend_numbers(new[0], refnet, n_qry)
        isolateClustering, merged_queries = network.print_cluster_numbers(
            numbers, rNames + qNames, output_fn, old_cluster_file, external_clustering,
            write_references or update_db, write_unwords=False)
        result.update(isolateClustering={'combined': isolateClustering}, merged_queries=merged_queries,
                      qqDistMat=qqDistMat)
        if return_network:
            parts = (network._cat([new[0], loaded[0]]), n_ref + n_qry)
            if len(new) > 2:
                parts += (network._cat([new[2], loaded[2]]),)
            result["genomeNetwork"] = parts
        return result

    if external_clustering is not None:
        raise NotImplementedError("assign_query_clusters: external clusters under serial / stable are not mirrored")
    if stable is not None:
        sys.stderr.write("Assigning stably\n")
        refClustering = readIsolateTypeFromCsv(old_cluster_file, mode='clusters', return_dict=True)['Cluster']
        dist_col = 0 if stable == "core" else 1
        ref_idxs = nearest_reference(qrDistMat, n_qry, n_ref, dist_col)
        qa = queryAssignments.cpu().numpy() if _is_cuda(queryAssignments) else np.asarray(queryAssignments)
        linked = qa[np.arange(n_qry, dtype=np.int64) * n_ref + ref_idxs] == -1
        isolateClustering = stable_names(rNames, qNames, ref_idxs, linked, refClustering)
    else:
        sys.stderr.write("Assigning serially\n")
        edges, _ = network.assignment_edges(queryAssignments, model.within_label, False, n_ref)
        degree, n_links, links = links_of(edges, refnet, n_qry, MAX_LINKS)
        isolateClustering = serial_names(rNames, qNames, degree, n_links, links, edges, refnet.labels,
                                         old_clusters_of(old_cluster_file))
    write_query_csv(isolateClustering, output)
    result["isolateClustering"] = isolateClustering
    return result


def assign_from_sketches(ref_db, qry_db, model, refnet, qNames, kmers, random_tbl, output, write_references=False,
                         external_clustering=None, file_extension_string='', printCSV=True, **kw):
    """Joint assignment straight from resident sketches (engine.SketchDB), the distance matrix never formed:
    model.edges_from_sketches (the fused distance -> edge path) for the query-reference edges, their degrees
    (query_links_dev), a query-query self job with the same model when a query is unlinked (addQueryToNetwork's rule
    and messages), ONE cluster_extend_dev over the new edges, and print_cluster_numbers for the names.  `model`:
    a RefineBoundary or BGMMModel; **kw goes to its edges_from_sketches (e.g. slope=0 for a core-refined fit).
    Returns (isolateClustering, merged_queries), as printClusters."""
    import torch
    from . import engine
    rNames, qNames = refnet.rNames, list(qNames)
    n_ref, n_qry = len(rNames), len(qNames)
    if ref_db.n != n_ref or qry_db.n != n_qry:
        raise ValueError("one name per sketch of each database")
    edges, _ = model.edges_from_sketches(ref_db, qry_db, kmers, random_tbl, **kw)
    labels_t = refnet.labels_on(edges.device)
    degree = engine.query_links_dev(edges, labels_t, n_qry, 1)[0]
    if bool((degree == 0).any().item()):
        sys.stderr.write("Found novel query clusters. Calculating distances between them.\n")
        if n_qry > 1:
            sys.stderr.write("Calculating all query-query distances\n")
            qq, _ = model.edges_from_sketches(qry_db, None, kmers, random_tbl, **kw)
            edges = torch.cat([qq + n_ref, edges])
    numbers, _ = engine.cluster_extend_dev(edges.contiguous(), labels_t, n_qry)
    output_fn = os.path.join(output, os.path.basename(output) + file_extension_string)
    return network.print_cluster_numbers(numbers.cpu().numpy(), rNames + qNames, output_fn, refnet.old_cluster_file,
                                         external_clustering, write_references, printCSV, write_unwords=False)
