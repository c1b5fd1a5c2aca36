#!/usr/bin/env python3
"""Generates tests/golden/bgmm_fit.npz: sklearn's BayesianGaussianMixture fits with fit2dMultiGaussian's settings
(PopPUNK/bgmm.py:38-43), from recorded initial labels, on the float64 image of float32 (already scaled) points.

Needs sklearn (1.7 here) and scipy; the fixture it writes is data only (points, labels, sklearn's results).

Per case: rs = check_random_state(seed); labels0 = KMeans(K, n_init=1, random_state=rs).fit(X64).labels_; then
BayesianGaussianMixture(..., n_init=1, random_state=seed).fit(X64), whose first initialisation draws the same k-means.
That it did is asserted: the numpy restatement of tests/test_bgmm_fit_host.py, run from labels0, must reproduce
sklearn's n_iter_, parameters and bound trace.  Recorded: weights_, means_, covariances_, weight_concentration_,
mean_precision_, degrees_of_freedom_, n_iter_, converged_, lower_bound_, lower_bounds_, and the same parameters after
initialisation only (max_iter=0), under `init_*`.

Two conditions on every committed case:
  stop margin   min_t | |bound_t - bound_{t-1}| - tol | >= 1e-6 over the run, so that n_iter does not hang on rounding;
                a seed that fails it is passed over
  order spread  the restatement on eight fixed permutations of the rows; `spread_par` / `spread_lb` are the largest
                difference in any fitted parameter / in the bound trace against sklearn's, over those and the
                unpermuted run (floored at 1e-15 / 1e-12 so that a tolerance derived from them is never zero)
Cases: distances of poppunk_amd.synth databases through the CPU oracle (as make_golden_bgmm.py builds them) and planted
blobs; K = 1 .. 8; `has_duplicates` marks the case with repeated points and (0, 0) rows.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TOL = 1e-3
KEYS = ("weights", "means", "covariances", "weight_concentration", "mean_precision", "degrees_of_freedom")


def synth_distances(cluster_size, n_rows, rng):
    from oracle import oracle
    from poppunk_amd import synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(240, kmers, cluster_size=cluster_size, seed=7)
    X, _ = oracle.query(sk, None, kmers, 16, 14, synth.random_match_table(kmers), threads=8)
    X = np.asarray(X, dtype=np.float32)
    X = X[rng.choice(X.shape[0], n_rows, replace=False)]
    return (X / np.amax(X, axis=0)).astype(np.float32)          # ClusterFit.fit's float32 division


def blobs(n, centres, sd, rng):
    per = [n // len(centres) + (1 if i < n % len(centres) else 0) for i in range(len(centres))]
    X = np.vstack([rng.normal(c, s, (m, 2)) for c, s, m in zip(centres, sd, per)])
    return np.abs(X[rng.permutation(n)]).astype(np.float32)


def sk_params(m):
    return {"weights": m.weights_, "means": m.means_, "covariances": m.covariances_,
            "weight_concentration": np.stack(m.weight_concentration_), "mean_precision": m.mean_precision_,
            "degrees_of_freedom": m.degrees_of_freedom_}


def sklearn_fit(X64, K, seed, max_iter=100):
    from sklearn.mixture import BayesianGaussianMixture
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return BayesianGaussianMixture(n_components=K, n_init=1, covariance_type="full", weight_concentration_prior=0.1,
                                       mean_precision_prior=0.1, mean_prior=np.array([0, 0]), max_iter=max_iter,
                                       random_state=seed).fit(X64)


def try_case(X32, K, seed):
    """The recorded arrays of one case, or None when the stop margin fails."""
    import test_bgmm_fit_host as H
    from sklearn.cluster import KMeans
    from sklearn.utils import check_random_state
    X64 = X32.astype(np.float64)
    labels0 = KMeans(n_clusters=K, n_init=1, random_state=check_random_state(seed)).fit(X64).labels_.astype(np.int32)
    m, m0 = sklearn_fit(X64, K, seed), sklearn_fit(X64, K, seed, max_iter=0)
    want = sk_params(m)
    trace = np.asarray(m.lower_bounds_, dtype=np.float64)
    steps = np.abs(np.diff(np.concatenate([[-np.inf], trace])))
    margin = float(np.abs(steps - TOL).min())
    if margin < 1e-6:
        return None
    spread_par, spread_lb = 1e-15, 1e-12
    rng = np.random.default_rng(1000 + seed)
    for p in range(9):
        perm = np.arange(X64.shape[0]) if p == 0 else rng.permutation(X64.shape[0])
        f = H.ref_fit(X64[perm], labels0[perm], K)
        assert f["n_iter"] == m.n_iter_ and f["converged"] == m.converged_, (f["n_iter"], m.n_iter_)
        spread_par = max(spread_par, H.worst(f, want))
        spread_lb = max(spread_lb, float(np.abs(f["lower_bounds"] - trace).max()))
        if p == 0:      # the restatement from labels0 IS sklearn's run: its first initialisation drew the same k-means
            # (the initial state agrees to rounding; up to 100 iterations amplify that, another draw differs at once)
            assert H.worst(H.ref_params(f["init"]), sk_params(m0)) < 1e-11, "labels0 is not sklearn's draw"
            assert H.worst(f, want) < 1e-6 and abs(f["lower_bound"] - m.lower_bound_) < 1e-5, "the run left sklearn's"
    out = dict(want, X=X32, K=np.asarray(K), seed=np.asarray(seed), labels0=labels0, n_iter=np.asarray(m.n_iter_),
               converged=np.asarray(bool(m.converged_)), lower_bound=np.asarray(m.lower_bound_), lower_bounds=trace,
               stop_margin=np.asarray(margin), spread_par=np.asarray(spread_par), spread_lb=np.asarray(spread_lb),
               has_duplicates=np.asarray(bool(np.unique(X32, axis=0).shape[0] < X32.shape[0])))
    out.update({"init_" + k: v for k, v in sk_params(m0).items()})
    return out


def main():
    rng = np.random.default_rng(20261016)
    three = ([0.08, 0.1], [0.45, 0.5], [0.8, 0.75])
    dup = blobs(1500, ([0.2, 0.25], [0.36, 0.42]), (0.07, 0.1), rng)          # two blobs that overlap
    dup = np.vstack([dup, dup[:700], np.zeros((25, 2), dtype=np.float32)])[rng.permutation(2225)]
    data = [("synth_k2", synth_distances(20, 5003, rng), 2), ("synth_k4", synth_distances(120, 6001, rng), 4),
            ("blobs_k1", blobs(2001, three[:1], (0.05,), rng), 1), ("blobs_k3", blobs(3001, three, (0.02, 0.05, 0.04), rng), 3),
            ("blobs_k6", blobs(4099, three, (0.03, 0.08, 0.06), rng), 6), ("blobs_k8", blobs(7001, three, (0.02, 0.1, 0.07), rng), 8),
            ("dups_k2", np.ascontiguousarray(dup), 2)]
    out, cases = {}, []
    for case, X, K in data:
        for seed in range(20):
            got = try_case(X, K, seed)
            if got is not None:
                break
        else:
            raise RuntimeError("no seed of %s keeps the stop margin" % case)
        cases.append(case)
        out.update({"%s_%s" % (case, k): v for k, v in got.items()})
        print("%-9s K %d n %5d seed %2d  n_iter %3d converged %-5s min weight %.4f  margin %.1e  spread par %.1e lb %.1e"
              % (case, K, X.shape[0], seed, got["n_iter"], bool(got["converged"]), got["weights"].min(),
                 got["stop_margin"], got["spread_par"], got["spread_lb"]))
    out["cases"] = np.asarray(cases)
    out["source"] = np.asarray("sklearn %s BayesianGaussianMixture / KMeans, executed by tests/golden/make_golden_bgmm_fit.py"
                               % __import__("sklearn").__version__)
    path = os.path.join(HERE, "bgmm_fit.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
