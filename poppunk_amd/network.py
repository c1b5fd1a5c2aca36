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
"""
import sys

import numpy as np

from . import refine

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
