"""generate_mst_from_sparse_input (PopPUNK/sparse_mst.py:82-119) on the MI355X.

    generate_mst_from_sparse_input(sparse_mat, rlist, old_rlist=None, previous_mst=None, gpu_graph=False)
        -> (edges int64 [k, 2], n_vertices, weights float64 [k])

The kNN graph of a lineage fit (construct_network_from_sparse_matrix: one weighted edge per stored entry, in COO order,
over len(rlist) vertices) and then network.generate_minimum_spanning_tree on it, as the reference's CPU branch.
`sparse_mat` is a scipy COO matrix (row, col, data) or the (i, j, dist) CUDA tensors of engine.knn_from_sketches /
knn_ref_query, read in place.  A kNN list holds (i, j) and (j, i) for mutual neighbours: both are kept as parallel
edges, as graph-tool keeps them.  `previous_mst` (not None) raises NotImplementedError; `old_rlist` and `gpu_graph`
are accepted and ignored.
"""
import numpy as np

from . import network


def _graph(sparse_mat, n):
    if isinstance(sparse_mat, (tuple, list)):
        i_t, j_t, w_t = sparse_mat
        if hasattr(i_t, "is_cuda"):
            import torch
            return torch.stack([i_t.to(torch.int64), j_t.to(torch.int64)], dim=1).contiguous(), n, \
                w_t.to(torch.float32).contiguous()
        return np.stack([np.asarray(i_t), np.asarray(j_t)], axis=1).astype(np.int64), n, np.asarray(w_t)
    coo = sparse_mat.tocoo()
    return np.stack([coo.row, coo.col], axis=1).astype(np.int64), n, np.asarray(coo.data)


def generate_mst_from_sparse_input(sparse_mat, rlist, old_rlist=None, previous_mst=None, gpu_graph=False):
    """PopPUNK/sparse_mst.py:82-119, CPU (graph-tool) branch, with the forest from the device."""
    if previous_mst is not None:
        raise NotImplementedError("generate_mst_from_sparse_input: previous_mst merging is not mirrored")
    return network.generate_minimum_spanning_tree(_graph(sparse_mat, len(rlist)), gpu_graph)
