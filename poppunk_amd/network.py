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
`betweenness_sample` and `use_gpu` only steer the reference's cugraph branch: accepted and ignored.  `subsample`
(random vertex subsampling) raises NotImplementedError before the device is touched.

Minimum spanning trees: generate_minimum_spanning_tree and generate_network_from_distances
(PopPUNK/network.py:1721-1831, 2075-2151) take and return G as (edges, n_vertices, weights); the forest comes from
ppk_mst / ppk_mst_dev and the seed linking (seed_links) runs on the host.
"""
import ctypes as C
import sys

import numpy as np

from . import _lib, refine

betweenness_sample_default = refine.betweenness_sample_default


def _counts(G, calc_betweenness):
    edges, n = G
    n = int(n)
    if hasattr(edges, "is_cuda"):
        from . import engine
        if calc_betweenness:
            stats, bt, _, _ = engine.network_summary_graph_dev(edges, n)
            return stats.cpu().numpy(), bt.cpu().numpy(), n
        stats, _ = engine.network_stats_dev(edges, n)
        return stats.cpu().numpy(), None, n
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if calc_betweenness:
        stats, bt, _, _ = refine.network_summary(e[:, 0], e[:, 1], None, n, 1)
        return stats[0], bt[0], n
    stats, _ = refine.network_sweep(e[:, 0], e[:, 1], np.zeros(e.shape[0], dtype=np.int64), n, 1)
    return stats[0], None, n


def networkSummary(G, calc_betweenness=True, betweenness_sample=betweenness_sample_default, subsample=None,
                   use_gpu=False):
    """PopPUNK/network.py:1204-1307, graph-tool branch (see the module docstring)."""
    if subsample is not None:
        raise NotImplementedError("networkSummary: random vertex subsampling (subsample) is not mirrored")
    stats, bt, n = _counts(G, calc_betweenness)
    return refine.summary_from_stats(stats, n, bt)


def print_network_summary(G, sample_size=None, betweenness_sample=betweenness_sample_default, use_gpu=False):
    """PopPUNK/network.py:616-643: networkSummary's metrics and scores to stderr, in the reference's words."""
    (metrics, scores) = networkSummary(G, subsample=sample_size, betweenness_sample=betweenness_sample,
                                       use_gpu=use_gpu)
    sys.stderr.write("Network summary:\n" + "\n".join(["\tComponents\t\t\t\t" + str(metrics[0]),
                                                       "\tDensity\t\t\t\t\t" + "{:.4f}".format(metrics[1]),
                                                       "\tTransitivity\t\t\t\t" + "{:.4f}".format(metrics[2]),
                                                       "\tMean betweenness\t\t\t" + "{:.4f}".format(metrics[3]),
                                                       "\tWeighted-mean betweenness\t\t" + "{:.4f}".format(metrics[4]),
                                                       "\tScore\t\t\t\t\t" + "{:.4f}".format(scores[0]),
                                                       "\tScore (w/ betweenness)\t\t\t" + "{:.4f}".format(scores[1]),
                                                       "\tScore (w/ weighted-betweenness)\t\t" + "{:.4f}".format(scores[2])])
                     + "\n")


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
