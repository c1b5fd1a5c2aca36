"""The silhouette rule (include/ppk.h "Silhouette") restated in numpy, operation for operation: the
float32 metric, q = rint(d * 2^shift) as int64, integer sums T[i][c] by np.add.at, then a, b, s in float64 in the order
the header lists.  The device results are compared with this bit for bit; this is compared with sklearn's arrays
(tests/golden/silhouette.npz) within the derived bound `bound`."""
import numpy as np


def shift_of(n):
    r = 0
    while r < 62 and (1 << r) < n:
        r += 1
    return min(40, 61 - r)


def samples_of(n_rows):
    n = int(round((1 + (1 + 8 * n_rows) ** 0.5) / 2))
    assert n * (n - 1) // 2 == n_rows
    return n


def metric_f32(x, metric):
    """float32 [n_rows] distances of the float32 [n_rows, 2] matrix, nothing fused."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x0, x1 = x[:, 0], x[:, 1]
    if metric == 0:
        return x0.copy()
    if metric == 1:
        return x1.copy()
    if metric == 2:
        return np.sqrt(x0 * x0 + x1 * x1)
    return np.abs(x0 - x1)


def square_f64(x, metric):
    """The float64 n x n matrix sklearn is given: the float32 metric, widened."""
    d = metric_f32(x, metric)
    n = samples_of(len(d))
    sq = np.zeros((n, n), dtype=np.float64)
    iu = np.triu_indices(n, 1)           # the condensed order: row i, then j ascending
    sq[iu] = d
    return sq + sq.T


def silhouette(x, levels, metric=2, shift=None):
    """(a, b, s float64 [n_levels, n], n_labels int32 [n_levels], valid int32 [n_levels])."""
    levels = np.atleast_2d(np.asarray(levels, dtype=np.int64))
    n_levels, n = levels.shape
    d = metric_f32(x, metric)
    assert samples_of(len(d)) == n
    if shift is None:
        shift = shift_of(n)
    q = np.rint(d.astype(np.float64) * 2.0 ** shift).astype(np.int64)
    qi, qj = np.triu_indices(n, 1)
    a = np.full((n_levels, n), np.nan)
    b = np.full((n_levels, n), np.nan)
    s = np.full((n_levels, n), np.nan)
    n_labels = np.zeros(n_levels, dtype=np.int32)
    valid = np.zeros(n_levels, dtype=np.int32)
    inv = 2.0 ** -shift
    for t in range(n_levels):
        lab = levels[t]
        cnt = np.bincount(lab, minlength=n + 1)
        n_labels[t] = np.count_nonzero(cnt)
        valid[t] = 1 if 2 <= n_labels[t] <= n - 1 else 0
        if not valid[t]:
            continue
        T = np.zeros((n, n + 1), dtype=np.int64)
        np.add.at(T, (qi, lab[qj]), q)
        np.add.at(T, (qj, lab[qi]), q)
        for i in range(n):
            ci = lab[i]
            if cnt[ci] == 1:
                a[t, i] = b[t, i] = s[t, i] = 0.0
                continue
            ai = (np.float64(T[i, ci]) * inv) / np.float64(cnt[ci] - 1)
            others = np.flatnonzero(cnt)
            others = others[others != ci]
            bi = np.min((T[i, others].astype(np.float64) * inv) / cnt[others].astype(np.float64))
            top = max(ai, bi)
            a[t, i], b[t, i] = ai, bi
            s[t, i] = 0.0 if top == 0.0 else (bi - ai) / top
    return a, b, s, n_labels, valid


def bound(x, metric, n, a_ref, b_ref, shift=None):
    """|s - s_sklearn| allowed per sample: eps = 2^-(shift + 1) + n * 2^-53 * max d bounds the difference of a and of b,
    so 4 * eps / max(a, b) bounds that of s where max(a, b) > 0; exactly 0 elsewhere."""
    if shift is None:
        shift = shift_of(n)
    d = metric_f32(x, metric)
    eps = 2.0 ** -(shift + 1) + n * 2.0 ** -53 * float(d.max())
    top = np.maximum(a_ref, b_ref)
    return eps, np.where(top > 0, 4.0 * eps / np.where(top > 0, top, 1.0), 0.0)


def same_bits(got, want):
    """np.array_equal on float64 arrays with the NaN cells compared by mask."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
