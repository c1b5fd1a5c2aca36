"""Writes tests/golden/silhouette.npz: small long-form matrices, labelings, and what
sklearn.metrics.silhouette_samples(X, labels, metric='precomputed') gives for X = the float64 square of each of the
four metrics (recorded with sklearn 1.7.2, numpy's float64 sums).  Beside every sklearn array the float64 means a, b it
rests on, restated here from the square (they set the denominator of the tests' bound).

    python tests/golden/make_golden_silhouette.py

The cases hold what the fixed point can get wrong: distances below 2^-17 (a float32 of at least 2^-17 is an exact
multiple of 2^-40, so larger values never round), exact zeros, duplicate samples, singletons, label numbers with gaps.
Checked here, on the CPU: max(a, b) >= 1e-6 for at least 90 % of the samples of every case and metric (but n = 3 and
n = 5, where one singleton is already a third or a fifth), so that the bound 4 * eps / max(a, b) is not vacuous; and
the numpy restatement (tests/silhouette_model.py) is within it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import silhouette_model as model      # noqa: E402


def long_form(n, groups, rng, within, between, tiny=False):
    """float32 [n(n-1)/2, 2]: core distances `within` a group and `between` groups (uniform in the given ranges, or
    log-uniform for `tiny` within-group distances), accessory distances five times wider, independently drawn."""
    i, j = np.triu_indices(n, 1)
    same = groups[i] == groups[j]
    x = np.empty((len(i), 2), dtype=np.float64)
    for col, mul in ((0, 1.0), (1, 5.0)):
        far = rng.uniform(between[0], between[1], len(i)) * mul
        if tiny:
            near = 2.0 ** rng.uniform(np.log2(within[0]), np.log2(within[1]), len(i))
        else:
            near = rng.uniform(within[0], within[1], len(i)) * mul
        x[:, col] = np.where(same, near, far)
    return np.minimum(x, 1.0).astype(np.float32)


def duplicate(x, n, src, dst):
    """Sample dst becomes a copy of sample src: the same distances to everyone, 0 between the two."""
    sq = [model.square_f64(x, m).astype(np.float32) for m in (0, 1)]
    for m in sq:
        m[dst, :] = m[src, :]
        m[:, dst] = m[:, src]
        m[dst, dst] = 0.0
        m[src, dst] = m[dst, src] = 0.0
    iu = np.triu_indices(n, 1)
    return np.stack([sq[0][iu], sq[1][iu]], axis=1)


def means(sq, labels):
    """a, b in float64 from the square: the intra-cluster mean over the others, the least mean to another cluster."""
    n = len(labels)
    a, b = np.zeros(n), np.zeros(n)
    names = np.unique(labels)
    for i in range(n):
        own = labels == labels[i]
        if own.sum() == 1:
            continue
        a[i] = sq[i, own].sum() / (own.sum() - 1)
        b[i] = min(sq[i, labels == c].mean() for c in names if c != labels[i])
    return a, b


def cases():
    rng = np.random.default_rng(20261019)
    out = []
    # 0: ordinary magnitudes, three clusters, two tiles plus a remainder
    n = 130
    g = rng.integers(0, 3, n)
    out.append((long_form(n, g, rng, (0.001, 0.01), (0.02, 0.06)), g + 1))
    # 1: within-cluster distances between 2^-36 and 2^-18, exact zeros, duplicate samples, three singletons
    n = 65
    g = rng.integers(0, 4, n)
    g[:3] = (4, 5, 6)
    x = long_form(n, g, rng, (2.0 ** -36, 2.0 ** -18), (0.01, 0.08), tiny=True)
    # (a zero to a singleton would make that sample's b zero: the zeros stay among the other samples)
    free = np.flatnonzero(np.triu_indices(n, 1)[0] >= 3)
    x[rng.choice(free, 40, replace=False)] = 0.0
    x[rng.choice(free, 20, replace=False), 0] = 0.0
    same = np.flatnonzero(g == g[10])
    x = duplicate(x, n, int(same[0]), int(same[1]))
    x = duplicate(x, n, int(same[2]), int(same[3]))
    out.append((x, g + 1))
    # 2: one large cluster, a few small ones, two singletons; label numbers with gaps {1, 5, 9, 33, 64}
    n = 64
    g = np.full(n, 1)
    g[40:50], g[50:62], g[62], g[63] = 5, 9, 33, 64
    out.append((long_form(n, g, rng, (0.0005, 0.004), (0.01, 0.03)), g))
    # 3, 4: the smallest shapes
    out.append((long_form(5, np.array([0, 0, 1, 1, 1]), rng, (0.001, 0.01), (0.02, 0.06)), np.array([2, 2, 5, 5, 5])))
    out.append((long_form(3, np.array([0, 0, 1]), rng, (0.001, 0.01), (0.02, 0.06)), np.array([1, 1, 3])))
    return out


def main():
    import sklearn
    from sklearn.metrics import silhouette_samples
    arrays = {"sklearn_version": np.array(sklearn.__version__), "n_cases": np.array(len(cases()))}
    for k, (x, labels) in enumerate(cases()):
        labels = labels.astype(np.int32)
        n = len(labels)
        assert x.dtype == np.float32 and x.min() >= 0.0 and x.max() <= 1.0
        arrays["case%d_x" % k], arrays["case%d_labels" % k] = x, labels
        for metric in range(4):
            sq = model.square_f64(x, metric)
            sk = silhouette_samples(sq, labels, metric="precomputed")
            a, b = means(sq, labels)
            arrays["case%d_sk%d" % (k, metric)] = sk
            arrays["case%d_a%d" % (k, metric)], arrays["case%d_b%d" % (k, metric)] = a, b
            share = float(np.mean(np.maximum(a, b) >= 1e-6))
            assert share >= 0.9 or n <= 5, (k, metric, share)
            ma, mb, ms, _, valid = model.silhouette(x, labels, metric)
            eps, allowed = model.bound(x, metric, n, a, b)
            assert valid[0] == 1
            assert np.abs(ma[0] - a).max() <= eps and np.abs(mb[0] - b).max() <= eps, (k, metric)
            assert np.all(np.abs(ms[0] - sk) <= allowed), (k, metric, float(np.abs(ms[0] - sk).max()))
            print("case %d metric %d: n %d, below 2^-17: %d, zeros: %d, max(a,b) >= 1e-6: %.2f, max |s - sklearn| %.3g, "
                  "model == sklearn bits: %s" % (k, metric, n, int(np.sum((model.metric_f32(x, metric) < 2.0 ** -17))),
                                                 int(np.sum(model.metric_f32(x, metric) == 0)), share,
                                                 float(np.abs(ms[0] - sk).max()), np.array_equal(ms[0], sk)))
    path = os.path.join(HERE, "silhouette.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
