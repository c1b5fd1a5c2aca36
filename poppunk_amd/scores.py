"""Silhouette scores of a clustering from the long-form distances: the job of
scripts/poppunk_calculate_silhouette.py, without the n x n matrix and for every level of a sweep in one device call.

    python -m poppunk_amd.scores --distances db/db.dists --cluster-csv db/db_clusters.csv [--metric euclidean]

* `silhouette_samples`, `silhouette_score` -- sklearn.metrics' pair of the same names for metric='precomputed', fed
  with the float32 [n(n-1)/2, 2] matrix instead of a square one.
* `silhouette_of_levels` -- the mean silhouette of every level of a family (rows of engine.cluster_sweep_dev), the call
  a boundary sweep or multi_refine makes to rank its clusterings.
* `calculate_silhouette` -- the script's arguments and errors.

The sums are integers on the device (ppk_silhouette_dev), so a score is the same bits on every run; a and b differ from
sklearn's float64 means by at most 2^-(shift + 1) + n * 2^-53 * max d.

External scores, between two clusterings of the same samples (the files' side is
poppunk_amd.rand_indices):

* `pair_confusion_matrix`, `rand_score`, `adjusted_rand_score` -- sklearn.metrics' functions of the same names, the
  same results float for float (sklearn 1.7.2), from the integer sums of ppk_contingency_sums.
* `rand_index_score` -- the function of scripts/poppunk_calculate_rand_indices.py.
* `rand_of_levels` -- the Rand and adjusted Rand matrices of every level of a family against every level of another
  (or itself) from one device call, and which level refines which.
"""
import csv
import ctypes as C
import re
import sys

import numpy as np

from . import _lib, distfile, engine

METRICS = {"core": 0, "accessory": 1, "euclidean": 2, "difference": 3}
LABEL_COUNT_MESSAGE = "Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)"


def metric_code(metric):
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, not %r" % (", ".join(repr(m) for m in METRICS), metric))
    return METRICS[metric]


def factorise(labels):
    """Any sequence of hashable cluster names -> (int32 [n] numbers in [1, n], by first appearance; the count)."""
    seen = {}
    numbers = np.empty(len(labels), dtype=np.int32)
    for k, name in enumerate(labels):
        numbers[k] = seen.setdefault(name, len(seen) + 1)
    return numbers, len(seen)


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _device_silhouette(distMat, levels, metric, device_id=0):
    """(s float64 [n_levels, n], n_labels, valid) as numpy arrays for int32 [n_levels, n] numbers: a CUDA matrix is
    read where it is (ppk_silhouette_dev), a numpy one goes through the host form (ppk_silhouette)."""
    levels = np.ascontiguousarray(levels, dtype=np.int32)
    if _is_tensor(distMat):
        import torch
        lv = torch.from_numpy(levels).to(distMat.device)
        s, n_labels, valid = engine.silhouette_dev(distMat, lv, metric=metric)
        return s.cpu().numpy(), n_labels.cpu().numpy(), valid.cpu().numpy()
    x = np.ascontiguousarray(distMat, dtype=np.float32)
    n_levels, n = levels.shape
    s = np.empty((n_levels, n), dtype=np.float64)
    n_labels = np.empty(n_levels, dtype=np.int32)
    valid = np.empty(n_levels, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = _lib.lib().ppk_silhouette(x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], int(metric),
                                   levels.ctypes.data_as(ip), n_levels, engine.silhouette_shift(n), int(device_id),
                                   None, None, s.ctypes.data_as(dp), n_labels.ctypes.data_as(ip),
                                   valid.ctypes.data_as(ip))
    _lib.check(rc, "ppk_silhouette")
    return s, n_labels, valid


def _samples(distMat):
    if len(distMat.shape) != 2 or distMat.shape[1] != 2:
        raise ValueError("distMat must be a long-form [n(n-1)/2, 2] matrix")
    return engine._samples_of(int(distMat.shape[0]))


def silhouette_samples(distMat, labels, metric="euclidean", device_id=0):
    """sklearn.metrics.silhouette_samples(X, labels, metric='precomputed') with X the square of `metric` ('core',
    'accessory', 'euclidean' = sqrt(core^2 + accessory^2) in float32, 'difference' = |core - accessory|), from the
    long-form matrix: a numpy array or a CUDA tensor.  labels: one hashable cluster name per sample.  Returns float64
    [n].  ValueError, in sklearn's words, unless there are 2 .. n - 1 distinct labels."""
    code = metric_code(metric)
    n = _samples(distMat)
    if len(labels) != n:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (n, len(labels)))
    numbers, n_labels = factorise(labels)
    if not 2 <= n_labels <= n - 1:
        raise ValueError(LABEL_COUNT_MESSAGE % n_labels)
    s, _, _ = _device_silhouette(distMat, numbers[None, :], code, device_id)
    return s[0]


def silhouette_score(distMat, labels, metric="euclidean", device_id=0):
    """sklearn.metrics.silhouette_score(..., metric='precomputed') without sampling: float(np.mean(samples))."""
    return float(np.mean(silhouette_samples(distMat, labels, metric=metric, device_id=device_id)))


def silhouette_of_levels(dist_t, levels_t, metric="euclidean"):
    """Mean silhouette of every level: dist_t the resident float32 [n(n-1)/2, 2] CUDA matrix, levels_t int32
    [n_levels, n] CUDA cluster numbers in [1, n] (engine.cluster_sweep_dev's rows).  Returns float64 [n_levels], NaN at
    the levels with fewer than 2 or more than n - 1 clusters."""
    s, _, _ = engine.silhouette_dev(dist_t, levels_t, metric=metric_code(metric))
    return np.array([np.mean(row) for row in s.cpu().numpy()], dtype=np.float64)


def _device_sums(levels_a, levels_b=None, device_id=0):
    """(sq_a, sq_b, labels_a, labels_b, sq_cells, n_cells) as numpy arrays for int32 [n_levels, n] numbers (levels_b
    None: B = A): CUDA tensors are read where they are (ppk_contingency_sums_dev), numpy arrays go through the host
    form (ppk_contingency_sums)."""
    if _is_tensor(levels_a):
        return tuple(t.cpu().numpy() for t in engine.contingency_sums_dev(levels_a, levels_b))
    a = np.ascontiguousarray(levels_a, dtype=np.int32)
    b = None if levels_b is None else np.ascontiguousarray(levels_b, dtype=np.int32)
    n_a, n = a.shape
    n_b = n_a if b is None else b.shape[0]
    sq_a, sq_b = np.empty(n_a, dtype=np.int64), np.empty(n_b, dtype=np.int64)
    labels_a, labels_b = np.empty(n_a, dtype=np.int32), np.empty(n_b, dtype=np.int32)
    sq_cells, n_cells = np.empty((n_a, n_b), dtype=np.int64), np.empty((n_a, n_b), dtype=np.int64)
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    rc = _lib.lib().ppk_contingency_sums(a.ctypes.data_as(ip), n_a, None if b is None else b.ctypes.data_as(ip), n_b, n,
                                         int(device_id), sq_a.ctypes.data_as(lp), sq_b.ctypes.data_as(lp),
                                         labels_a.ctypes.data_as(ip), labels_b.ctypes.data_as(ip),
                                         sq_cells.ctypes.data_as(lp), n_cells.ctypes.data_as(lp))
    _lib.check(rc, "ppk_contingency_sums")
    return sq_a, sq_b, labels_a, labels_b, sq_cells, n_cells


def _pair_sums(labels_true, labels_pred, device_id=0):
    """(n, S_true, S_pred, S_xy, K_true, K_pred) as Python integers for two labelings of any hashable names: the sums
    of the squared class sizes and of the squared cells of the contingency table, and the label counts."""
    n = len(labels_true)
    if len(labels_pred) != n:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (n, len(labels_pred)))
    if n == 0:
        return 0, 0, 0, 0, 0, 0
    sq_a, sq_b, labels_a, labels_b, sq_cells, _ = _device_sums(factorise(labels_true)[0][None, :],
                                                               factorise(labels_pred)[0][None, :], device_id)
    return n, int(sq_a[0]), int(sq_b[0]), int(sq_cells[0, 0]), int(labels_a[0]), int(labels_b[0])


def _confusion(n, s_true, s_pred, s_xy):
    """sklearn's pair_confusion_matrix from the sums, as Python integers (tn, fp, fn, tp)."""
    fp, fn = s_pred - s_xy, s_true - s_xy
    return n * n - fp - fn - s_xy, fp, fn, s_xy - n


def _rand(n, s_true, s_pred, s_xy):
    """sklearn 1.7.2's rand_score: int64 numerator and denominator, one float64 division."""
    tn, fp, fn, tp = (np.int64(v) for v in _confusion(n, s_true, s_pred, s_xy))
    numerator, denominator = tn + tp, tn + fp + fn + tp
    if numerator == denominator or denominator == 0:
        return 1.0
    return float(numerator / denominator)


def _adjusted_rand(n, s_true, s_pred, s_xy):
    """sklearn 1.7.2's adjusted_rand_score: Python integers, then its one expression."""
    tn, fp, fn, tp = _confusion(n, s_true, s_pred, s_xy)
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def _rand_index(n, s_true, s_pred, s_xy, k_true, k_pred):
    """The reference script's rand_index_score: its three perfect-match cases, then its expression in its order, the
    sums int64 and comb(n, 2) the float64 scipy.special.comb returns ((n - 1) * n in float64, halved)."""
    if k_true == k_pred == 1 or k_true == k_pred == 0 or k_true == k_pred == n:
        return 1.0
    n_samples_comb = np.float64(n - 1) * np.float64(n) / np.float64(2.0)
    return 1 + (np.int64(s_xy) - 0.5 * np.int64(s_true) - 0.5 * np.int64(s_pred)) / n_samples_comb


def pair_confusion_matrix(labels_true, labels_pred, device_id=0):
    """sklearn.metrics.cluster.pair_confusion_matrix: int64 [2, 2], C[1, 1] = S_xy - n, C[0, 1] = S_pred - S_xy,
    C[1, 0] = S_true - S_xy, C[0, 0] the rest of n^2 - n, from the device's sums.  Labels: any hashable names, one per
    sample.  ValueError, in sklearn's words, for labelings of unequal lengths."""
    n, s_true, s_pred, s_xy, _, _ = _pair_sums(labels_true, labels_pred, device_id)
    tn, fp, fn, tp = _confusion(n, s_true, s_pred, s_xy)
    return np.array([[tn, fp], [fn, tp]], dtype=np.int64)


def rand_score(labels_true, labels_pred, device_id=0):
    """sklearn.metrics.rand_score, the same float."""
    return _rand(*_pair_sums(labels_true, labels_pred, device_id)[:4])


def adjusted_rand_score(labels_true, labels_pred, device_id=0):
    """sklearn.metrics.adjusted_rand_score (1.7.2), the same float: Python integers, one true division, 1.0 where
    fn == fp == 0."""
    return _adjusted_rand(*_pair_sums(labels_true, labels_pred, device_id)[:4])


def rand_index_score(labels_true, labels_pred, device_id=0):
    """rand_index_score of scripts/poppunk_calculate_rand_indices.py, the same float: 1.0 where both labelings have one
    cluster, none, or n; otherwise 1 + (S_xy - 0.5 S_true - 0.5 S_pred) / comb(n, 2)."""
    return _rand_index(*_pair_sums(labels_true, labels_pred, device_id))


def rand_of_levels(levels_t, other_t=None):
    """(rand, adjusted, refines) for every level of levels_t against every level of other_t (None: of levels_t itself),
    from one device call: int32 [n_levels, n] CUDA cluster numbers in [1, n] (engine.cluster_sweep_dev's rows).  rand
    and adjusted are float64 [n_a, n_b], sklearn's rand_score and adjusted_rand_score of each pair; refines is bool
    [n_a, n_b]: level x of the first family refines level y of the second (no cluster of x is split by y), exactly."""
    sq_a, sq_b, labels_a, _, sq_cells, n_cells = _device_sums(levels_t, other_t)
    n = int(levels_t.shape[1])
    rand = np.empty(sq_cells.shape, dtype=np.float64)
    adjusted = np.empty(sq_cells.shape, dtype=np.float64)
    for x in range(sq_cells.shape[0]):
        for y in range(sq_cells.shape[1]):
            sums = (n, int(sq_a[x]), int(sq_b[y]), int(sq_cells[x, y]))
            rand[x, y], adjusted[x, y] = _rand(*sums), _adjusted_rand(*sums)
    return rand, adjusted, n_cells == labels_a.astype(np.int64)[:, None]


def read_cluster_csv(cluster_csv, cluster_col=2, id_col=1, sub=None):
    """The script's reading of its CSV (pd.read_csv(index_col=id_col - 1, quotechar='"'), then
    clustering.loc[sample][cluster_col - 2]): a header line; the id column is id_col - 1; the cluster column is taken by
    position cluster_col - 2 among the REMAINING columns.  `sub` is stripped from the ids.  Returns {id: cluster name};
    names are compared as the strings the file holds."""
    out = {}
    with open(cluster_csv, newline="") as f:
        rows = csv.reader(f, quotechar='"')
        next(rows, None)
        for row in rows:
            if not row:
                continue
            name = row[id_col - 1]
            rest = row[:id_col - 1] + row[id_col:]
            if sub is not None:
                name = re.sub(pattern=sub, repl="", string=name)
            out[name] = rest[cluster_col - 2]
    return out


def calculate_silhouette(distances, cluster_csv, cluster_col=2, id_col=1, sub=None, metric="euclidean", device_id=0):
    """scripts/poppunk_calculate_silhouette.py with its arguments: `distances` the prefix of the .pkl / .npy pair
    (RuntimeError unless it holds self-self distances), `cluster_csv` the assignments, `sub` a pattern removed from the
    sample names of both.  A sample the CSV lacks is a KeyError, as the script's clustering.loc[sample].  Returns the
    score.

    The script's own distance is euclidean(distRow[0], distRow[1]) on two SCALARS: under scipy releases whose
    `euclidean` accepted scalars that is |core - accessory|, metric='difference' here ([EXT]: not recorded, no such
    scipy at hand); under scipy 1.15.3 the line raises "ValueError: Input vector should be 1-D" and the script cannot
    run.  The default, 'euclidean', is the distance the line's name promises and process_weights uses."""
    rlist, _, is_self, X = distfile.readPickle(distances)
    if not is_self:
        raise RuntimeError("Distance DB should be self-self distances")
    if sub is not None:
        rlist = [re.sub(pattern=sub, repl="", string=name) for name in rlist]
    clustering = read_cluster_csv(cluster_csv, cluster_col, id_col, sub)
    labels = [clustering[sample] for sample in rlist]
    return silhouette_score(X, labels, metric=metric, device_id=device_id)


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Calculate Silhouette Coefficient for a clustering",
                                     prog="calculate_silhouette")
    parser.add_argument("--distances", required=True, help="Prefix of input pickle of pre-calculated distances (required)")
    parser.add_argument("--cluster-csv", required=True, help="Cluster assignments")
    parser.add_argument("--cluster-col", type=int, default=2, help="Column with cluster assignment (default = 2)")
    parser.add_argument("--id-col", type=int, default=1, help="Column with sample names (default = 1)")
    parser.add_argument("--sub", type=str, default=None, help="Remove string from sample names")
    parser.add_argument("--metric", choices=sorted(METRICS), default="euclidean",
                        help="Distance of a pair (default = euclidean)")
    parser.add_argument("--device", type=int, default=0, help="GPU to use (default = 0)")
    args = parser.parse_args(argv)
    print(calculate_silhouette(args.distances, args.cluster_csv, args.cluster_col, args.id_col, args.sub, args.metric,
                               args.device))


if __name__ == "__main__":
    sys.exit(main())
