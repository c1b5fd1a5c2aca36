#!/usr/bin/env python3
"""Generates tests/golden/bgmm_assign.npz, and with `--k` tests/golden/bgmm_assign_k.npz instead: BGMM assignment as
the reference computes it.  (Each file is written by its own entry point, so that one is never regenerated for the
other's sake.)

Run in the BUILD container only (needs the reference checkout and sklearn); the fixture it writes is data (model
arrays, input rows, expected outputs) and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast`, as make_golden.py does, and run under the real
numpy / scipy / sklearn of this image; nothing is restated):
  PopPUNK/bgmm.py     fit2dMultiGaussian, findWithinLabel, findBetweenLabel_bgmm, log_likelihood,
                      log_multivariate_normal_density
  PopPUNK/models.py   assign_samples (its BGMMFit branch: models.py:177-187), called with a stand-in BGMMFit that
                      carries the fitted arrays

Cases (prefix `<case>_` on every array; `cases` lists them, `raise_cases` the fits the reference refuses):
  k2, k4     sklearn fits with fit2dMultiGaussian's settings on synthetic distances (poppunk_amd.synth + the CPU
             oracle), scaled as ClusterFit.fit does (float32 np.amax); numpy's global seed is fixed before each fit.
             k4 is fitted on fewer, larger clusters, where the Dirichlet-process prior leaves one component
             near-empty (weight 0.003)
  k2_f64     the k2 fit with its scale stored as float64 (X / scale is then a float64 quotient)
  split_f32, split_f64
             a hand-made two-component model whose boundary is the line xs = 0.55, and rows on which the float32
             and the float64 quotient x / scale fall on opposite sides of it: the two cases' labels differ there
  jitter     a hand-made singular covariance: the 1e-7 fallback of log_multivariate_normal_density
  raise      a covariance that is not positive-definite even with the fallback (ValueError)
Rows of every case: a sample of the fit's own rows, the 10 x 10 grid of test/test-refine.py:47-50, (0, 0) failed
pairs, the component means (un-scaled) and far outliers.  Expected: labels (int64), float32 responsibilities, and
each row's gap between its two largest lpr.

Cases of bgmm_assign_k.npz (`--k`, main_k; the same array names per case): the component counts bgmm_assign.npz
does not hold, each with an ODD row count (a row is dropped where needed)
  k1         hand-made, one component: label 0 and responsibility 1.0 on every row, so every row is an edge
  k3         fit2dMultiGaussian(Xs, 3) on the synthetic distances (clusters of 60), float32 np.amax scale,
             np.random.seed(1) before the fit; within / between as findWithinLabel / findBetweenLabel_bgmm give them
  k3_f64     the k3 fit with its scale stored as float64
  k5, k16    hand-made (handmade()): means spread over [0, 1]^2, correlated covariances with correlations from -0.9
             to 0.9, one component of weight 1e-4; within = K - 1.  At most 1 200 of the fit's own rows (the
             responsibilities of 16 components are what fills the file), then the grid, zeros, means and far rows
main_k asserts, and writes nothing otherwise, that no row of any case is undecided (gap <= 1e-9 max(1, |top|), the
rule of tests/test_gpu_bgmm.py; an undecided row of the sklearn fit would be dropped), that every component of k3
and k5 and at least 12 of k16's are some row's label, and that the file is no larger than bgmm_assign.npz.
"""
import ast
import contextlib
import os
import sys

import numpy as np

REF = os.environ.get("POPPUNK_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def extract_functions(path, names, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    missing = [n for n in names if n not in namespace]
    if missing:
        raise RuntimeError("not found in %s: %s" % (path, missing))
    return namespace


class BGMMFit:
    """Stand-in carrying what assign_samples reads (weights, means, covariances)."""

    def __init__(self, weights, means, covariances):
        self.weights, self.means, self.covariances = weights, means, covariances


class _Absent:
    pass


def reference_namespace():
    import operator
    from scipy import linalg
    from scipy.special import logsumexp
    from sklearn import mixture
    ns = {"np": np, "linalg": linalg, "sp_logsumexp": logsumexp, "mixture": mixture, "operator": operator,
          "BGMMFit": BGMMFit, "DBSCANFit": _Absent, "NumpyShared": _Absent,
          "set_env": lambda **kw: contextlib.nullcontext()}
    extract_functions(os.path.join(REF, "PopPUNK", "bgmm.py"),
                      ["fit2dMultiGaussian", "findWithinLabel", "findBetweenLabel_bgmm", "log_likelihood",
                       "log_multivariate_normal_density"], ns)
    extract_functions(os.path.join(REF, "PopPUNK", "models.py"), ["assign_samples"], ns)
    return ns


def distances(cluster_size):
    from oracle import oracle
    from poppunk_amd import synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(240, kmers, cluster_size=cluster_size, seed=7)
    tbl = synth.random_match_table(kmers)
    X, _ = oracle.query(sk, None, kmers, 16, 14, tbl, threads=8)
    return np.asarray(X, dtype=np.float32)


def rows_for(X, means, scale, rng, n_own=3000):
    own = X[rng.choice(X.shape[0], n_own, replace=False)]
    g = np.arange(0, 1, 0.1, dtype=np.float32)
    xv, yv = np.meshgrid(g, g)
    grid = np.hstack((xv.reshape(-1, 1), yv.reshape(-1, 1)))
    zeros = np.zeros((4, 2), dtype=np.float32)
    on_means = (np.asarray(means) * np.asarray(scale, dtype=np.float64)).astype(np.float32)
    far = np.array([[5, 5], [1, 0], [0, 1], [0.99, 0.99], [50, 0.001], [1e-6, 1e-6]], dtype=np.float32)
    return np.ascontiguousarray(np.vstack([own, grid, zeros, on_means, far]), dtype=np.float32)


def expected(ns, X, weights, means, covariances, scale):
    model = BGMMFit(weights, means, covariances)
    n = X.shape[0]
    y = np.zeros(n, dtype=int)
    ns["assign_samples"](0, X, y, model, scale, n, values=False)
    resp = np.zeros((n, len(weights)), dtype=X.dtype)
    ns["assign_samples"](0, X, resp, model, scale, n, values=True)
    _, lpr = ns["log_likelihood"](X, weights, means, covariances, scale)
    top = np.sort(lpr, axis=1)
    gap = top[:, -1] - top[:, -2] if lpr.shape[1] > 1 else np.full(n, np.inf)
    return y.astype(np.int64), resp, gap, top[:, -1]


def record(ns, out, case, weights, means, covariances, sc, rows):
    labels, resp, gap, top = expected(ns, rows, weights, means, covariances, sc)
    for k, v in (("weights", weights), ("means", means), ("covariances", covariances), ("scale", sc),
                 ("X", rows), ("labels", labels), ("resp", resp), ("gap", gap), ("top", top)):
        out["%s_%s" % (case, k)] = np.asarray(v)
    return labels


def main():
    ns = reference_namespace()
    rng = np.random.default_rng(20261015)
    out = {}
    cases, raise_cases = [], []

    def add(case, weights, means, covariances, sc, rows):
        cases.append(case)
        return record(ns, out, case, weights, means, covariances, sc, rows)

    for case, K, cluster_size in (("k2", 2, 20), ("k4", 4, 120)):
        X = distances(cluster_size)
        scale = np.amax(X, axis=0)                 # ClusterFit.fit: float32 np.amax of the float32 matrix
        Xs = X / scale
        np.random.seed(1)                          # (sklearn draws its initialisations from numpy's global state)
        dpgmm = ns["fit2dMultiGaussian"](Xs, K)
        w, m, c = dpgmm.weights_, dpgmm.means_, dpgmm.covariances_
        y = np.zeros(Xs.shape[0], dtype=int)
        ns["assign_samples"](0, Xs, y, BGMMFit(w, m, c), np.array([1.0, 1.0]), Xs.shape[0])
        within = ns["findWithinLabel"](m, y)
        between = ns["findBetweenLabel_bgmm"](m, y)
        rows = rows_for(X, m, scale, rng)
        add(case, w, m, c, scale, rows)
        out[case + "_within"] = np.asarray(within)
        out[case + "_between"] = np.asarray(between)
        print("%s: weights %s within %d between %d" % (case, np.array2string(w, precision=4), within, between))
        if case == "k2":
            add("k2_f64", w, m, c, scale.astype(np.float64), rows)
            out["k2_f64_within"], out["k2_f64_between"] = np.asarray(within), np.asarray(between)

    # float32 against float64 quotient: rows within a float32 rounding of the boundary xs = 0.55 whose two quotients
    # fall on opposite sides of it (and at least 1e-9 away, so the reference's lpr gap is far above any tie)
    w = np.array([0.5, 0.5])
    m = np.array([[0.3, 0.5], [0.8, 0.5]])
    c = np.array([np.eye(2) * 0.01, np.eye(2) * 0.01])
    # a float32 quotient near 0.55 is one of a few float32 values, so only the one or two float32 distances closest to
    # 0.55 * scale can qualify: draw scales until one has them
    cand = np.zeros(0, dtype=np.float32)
    while cand.size == 0:
        sc32 = np.array([rng.uniform(0.02, 0.05), 0.0517], dtype=np.float32)
        c0 = np.float32(np.float64(0.55) * np.float64(sc32[0]))
        cand = np.array([np.nextafter(c0, np.float32(np.inf * k)) if k else c0 for k in (-1, 0, 1)], dtype=np.float32)
        q32 = (cand / sc32[0]).astype(np.float64)
        q64 = cand.astype(np.float64) / np.float64(sc32[0])
        cand = cand[((q32 - 0.55) * (q64 - 0.55) < 0) & (np.abs(q32 - 0.55) > 1e-9) & (np.abs(q64 - 0.55) > 1e-9)]
    near = np.stack([cand, np.full(cand.size, 0.5 * sc32[1], dtype=np.float32)], axis=1)
    rows = np.ascontiguousarray(np.vstack([near, rows_for(X, m, sc32, rng)[-200:]]), dtype=np.float32)
    for case, sc in (("split_f32", sc32), ("split_f64", sc32.astype(np.float64))):
        add(case, w, m, c, sc, rows)
        out[case + "_within"], out[case + "_between"] = np.asarray(0), np.asarray(1)
    out["split_rows"] = np.asarray(cand.size)

    # hand-made: component 0 singular (rank one) -> chol fails, cov + 1e-7 I is positive-definite
    w = np.array([0.5, 0.5])
    m = np.array([[0.2, 0.3], [0.7, 0.6]])
    c = np.array([[[1.0, 1.0], [1.0, 1.0]], [[0.02, 0.004], [0.004, 0.03]]])      # (exact in any factorisation order)
    rows = rows_for(X, m, scale, rng)
    add("jitter", w, m, c, scale, rows)
    out["jitter_within"], out["jitter_between"] = np.asarray(0), np.asarray(1)
    # not positive-definite even with the fallback: the reference raises ValueError
    c_bad = np.array([[[-0.01, 0.0], [0.0, 0.01]], [[0.02, 0.004], [0.004, 0.03]]])
    try:
        ns["log_likelihood"](rows[:4], w, m, c_bad, scale)
        raise RuntimeError("the reference accepted a covariance it should refuse")
    except ValueError:
        pass
    for k, v in (("weights", w), ("means", m), ("covariances", c_bad), ("scale", scale)):
        out["raise_%s" % k] = np.asarray(v)
    out["raise_within"], out["raise_between"] = np.asarray(0), np.asarray(1)
    raise_cases.append("raise")

    out["cases"] = np.asarray(cases)
    out["raise_cases"] = np.asarray(raise_cases)
    out["source"] = np.asarray("PopPUNK/bgmm.py fit2dMultiGaussian / findWithinLabel / findBetweenLabel_bgmm / "
                               "log_likelihood / log_multivariate_normal_density and PopPUNK/models.py "
                               "assign_samples, executed by tests/golden/make_golden_bgmm.py")
    path = os.path.join(HERE, "bgmm_assign.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "cases", cases)


def undecided(gap, top):
    """The rows test_gpu_bgmm.py leaves out of its label comparison: the two largest lpr within 1e-9 of a tie."""
    return gap <= 1e-9 * np.maximum(1.0, np.abs(top))


def handmade(K, rng):
    """K components for the run-time component loop: means spread over [0, 1]^2 (a Halton sequence, bases 2 and 3),
    standard deviations about a quarter of the means' spacing, correlations from -0.9 to 0.9 in a drawn order, drawn
    weights.  Component K // 2 has weight 1e-4 and is narrow (sd 0.004), so that it still owns the rows at its mean."""
    def halton(i, base):
        f, r = 1.0, 0.0
        while i > 0:
            f /= base
            r += f * (i % base)
            i //= base
        return r

    means = np.array([[0.05 + 0.9 * halton(i + 1, 2), 0.05 + 0.9 * halton(i + 1, 3)] for i in range(K)])
    rho = rng.permutation(np.linspace(-0.9, 0.9, K))
    sd = (0.25 / np.sqrt(K)) * rng.uniform(0.6, 1.4, size=(K, 2))
    tiny = K // 2
    sd[tiny] = 0.004
    w = rng.uniform(0.5, 1.5, size=K)
    w[tiny] = 0.0
    w *= (1.0 - 1e-4) / w.sum()
    w[tiny] = 1e-4
    cov = np.empty((K, 2, 2))
    for c in range(K):
        off = rho[c] * sd[c, 0] * sd[c, 1]
        cov[c] = [[sd[c, 0] ** 2, off], [off, sd[c, 1] ** 2]]
    return w, means, cov


def odd_rows(rows):
    return rows if rows.shape[0] % 2 else np.ascontiguousarray(rows[:-1])


def main_k():
    """tests/golden/bgmm_assign_k.npz: the component counts and the odd row counts bgmm_assign.npz does not hold."""
    ns = reference_namespace()
    rng = np.random.default_rng(20261019)
    out = {}
    cases = []
    n_labelled = {}

    def add(case, weights, means, covariances, sc, rows, within, between):
        rows = odd_rows(rows)
        labels = record(ns, out, case, weights, means, covariances, sc, rows)
        tie = undecided(out[case + "_gap"], out[case + "_top"])
        if tie.any():
            if case not in ("k3", "k3_f64"):
                raise RuntimeError("%s: %d undecided rows in a hand-made model" % (case, tie.sum()))
            rows = odd_rows(np.ascontiguousarray(rows[~tie]))       # (a fit's undecided rows leave the case)
            labels = record(ns, out, case, weights, means, covariances, sc, rows)
        out[case + "_within"], out[case + "_between"] = np.asarray(within), np.asarray(between)
        # the two conditions the fixture is committed under, and the odd row count
        assert rows.shape[0] % 2 == 1, case
        assert not undecided(out[case + "_gap"], out[case + "_top"]).any(), case
        n_labelled[case] = np.unique(labels).size
        cases.append(case)
        print("%s: %d rows, %d of %d components label a row, within %d between %d"
              % (case, rows.shape[0], n_labelled[case], len(weights), within, between))

    X = distances(60)
    scale = np.amax(X, axis=0)
    Xs = X / scale
    np.random.seed(1)
    dpgmm = ns["fit2dMultiGaussian"](Xs, 3)
    w3, m3, c3 = dpgmm.weights_, dpgmm.means_, dpgmm.covariances_
    y = np.zeros(Xs.shape[0], dtype=int)
    ns["assign_samples"](0, Xs, y, BGMMFit(w3, m3, c3), np.array([1.0, 1.0]), Xs.shape[0])
    within3, between3 = ns["findWithinLabel"](m3, y), ns["findBetweenLabel_bgmm"](m3, y)
    print("k3: weights %s" % np.array2string(w3, precision=4))

    w1, m1, c1 = np.array([1.0]), np.array([[0.4, 0.5]]), np.array([[[0.05, 0.01], [0.01, 0.04]]])
    add("k1", w1, m1, c1, scale, rows_for(X, m1, scale, rng), 0, 0)
    rows3 = rows_for(X, m3, scale, rng)
    add("k3", w3, m3, c3, scale, rows3, within3, between3)
    add("k3_f64", w3, m3, c3, scale.astype(np.float64), rows3, within3, between3)
    for K, n_own in ((5, 1200), (16, 650)):
        w, m, c = handmade(K, rng)
        add("k%d" % K, w, m, c, scale, rows_for(X, m, scale, rng, n_own), K - 1, 0)

    assert n_labelled["k3"] == 3 and n_labelled["k3_f64"] == 3 and n_labelled["k5"] == 5, n_labelled
    assert n_labelled["k16"] >= 12, n_labelled
    out["cases"] = np.asarray(cases)
    out["source"] = np.asarray("PopPUNK/bgmm.py fit2dMultiGaussian / findWithinLabel / findBetweenLabel_bgmm / "
                               "log_likelihood / log_multivariate_normal_density and PopPUNK/models.py "
                               "assign_samples, executed by tests/golden/make_golden_bgmm.py --k")
    path = os.path.join(HERE, "bgmm_assign_k.npz")
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    size, limit = os.path.getsize(tmp), os.path.getsize(os.path.join(HERE, "bgmm_assign.npz"))
    if size > limit:
        os.remove(tmp)
        raise RuntimeError("%d bytes: larger than bgmm_assign.npz (%d)" % (size, limit))
    os.replace(tmp, path)
    print("wrote", path, "cases", cases, "%d bytes (bgmm_assign.npz: %d)" % (size, limit))


if __name__ == "__main__":
    if sys.argv[1:] == ["--k"]:
        main_k()
    elif sys.argv[1:]:
        sys.exit("usage: make_golden_bgmm.py [--k]")
    else:
        main()
