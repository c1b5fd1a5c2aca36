"""GPU tests of the BGMM fit (include/ppk.h "BGMM fit") against the numpy restatement of
tests/test_bgmm_fit_host.py and sklearn's recorded fits (tests/golden/bgmm_fit.npz).

Bars.  Fits from the fixture's labels: 100 x the case's recorded order spread (the restatement's own sensitivity to
the order of the rows), the margin being for a reduction tree of another shape and device exp / log that differ from
libm by an ulp or two, carried through up to 100 iterations.  One pass (no iteration to amplify anything): 1e-11 of
each quantity's own scale -- nk and xk their own value, S r log r its value but at least 1, an entry of sk the geometric mean of the two
variances it sits between (an off-diagonal entry may cancel to nothing; its terms do not).  n eps = 1.6e-12 for the
largest case is the worst a re-ordered sum of n terms of that scale can do, and the ulp-level differences of exp /
log enter each term once, times |log r| for a small r.  The differences seen are printed (run with -s)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_bgmm_fit_host as H  # noqa: E402

from poppunk_amd import _lib, bgmm, engine  # noqa: E402
from poppunk_amd.models import BGMMModel, DBSCANModel  # noqa: E402

pytestmark = pytest.mark.gpu
ONE = (1.0, 1.0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in H.PARAM_KEYS + ("lower_bounds",)) and \
        (a.n_iter, a.converged, a.best_init) == (b.n_iter, b.converged, b.best_init)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embed(X, seed, scale=ONE):
    """X's rows (times scale) at random places of a larger matrix whose other rows hold anything, NaN included."""
    rng = np.random.default_rng(seed)
    n = X.shape[0]
    big = rng.uniform(0, 2, (n * 2 + 37, 2)).astype(np.float32)
    big[::5] = np.nan
    idx = rng.permutation(big.shape[0])[:n]
    big[idx] = X
    return big, idx.astype(np.int64)


def moments(sums, pivot):
    """nk, xk, sk (without reg_covar), S r log r of one pass's sums."""
    nk = sums[:, 0] + 10 * H.EPS
    m = sums[:, 1:3] / nk[:, None]
    f = 2.0 - sums[:, 0] / nk
    sk = np.stack([sums[:, 3] / nk - m[:, 0] * m[:, 0] * f, sums[:, 4] / nk - m[:, 0] * m[:, 1] * f,
                   sums[:, 5] / nk - m[:, 1] * m[:, 1] * f], axis=1)
    return nk, pivot + m, sk, sums[:, 6]


def close(got, want, bar=1e-11, scale=None):
    """(largest |got - want| / scale, whether it is within bar); scale: |want| unless given; where it is 0 the two must
    be equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), want.shape)
    err = np.abs(got - want)
    if np.any(err[scale == 0] != 0):
        return np.inf, False
    d = float((err[scale > 0] / scale[scale > 0]).max()) if np.any(scale > 0) else 0.0
    return d, d <= bar


def sk_scale(sk):
    """Per entry (xx, xy, yy) of sk [K, 3]: the geometric mean of the two variances around it."""
    return np.stack([sk[:, 0], np.sqrt(sk[:, 0] * sk[:, 2]), sk[:, 2]], axis=1)


def pass_close(got_sums, want_sums, pivot, what=None):
    """One pass's sums against the restatement's, quantity by quantity, each on its own scale."""
    got, want = moments(got_sums, pivot), moments(want_sums, pivot)
    # (log r = w - logsumexp w is a difference of log-probabilities tens to hundreds in size: each row's term carries an
    #  absolute eps |w| however small r log r itself is, so its scale is not allowed below 1)
    for name, a, b, scale in zip(("nk", "xk", "sk", "r log r"), got, want,
                                 (None, None, sk_scale(want[2]), np.maximum(1.0, np.abs(want[3])))):
        d, ok = close(a, b, scale=scale)
        if what:
            print("%s %-7s max |d| / scale = %.2e" % (what, name, d))
        assert ok, (what, name, d)


def k16_state(X):
    """A 16-component state: the restatement's first iteration from arbitrary labels."""
    labels = (np.arange(X.shape[0]) * 7 % 16).astype(np.int32)
    return H.ref_fit(X, labels, 16, max_iter=1)["first"]


# ---- 1. one statistics pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", [("blobs_k1", 1), ("synth_k2", 2), ("synth_k4", 4), ("blobs_k6", 6), ("blobs_k8", 8),
                                    ("blobs_k8", 16), ("dups_k2", 2)])
def test_one_pass_equals_the_restatement(case, K):
    g = H.case_of(H.golden(), case)
    X32 = g["X"]
    X = X32.astype(np.float64)
    assert X.shape[0] % 256 != 0
    S = k16_state(X) if K == 16 else H.ref_fit(X, g["labels0"], K, max_iter=1)["init"]
    st = H.state_from_ref(S, K)
    lr = H.ref_log_resp(X, S)
    want = H.ref_sums(X, np.exp(lr), lr, S["means"])
    got_c = engine.bgmm_stats_dev(cuda(X32), st, ONE).cpu().numpy()
    big, idx = embed(X32, 3)
    got_i = engine.bgmm_stats_dev(cuda(big), st, ONE, index_t=cuda(idx)).cpu().numpy()
    assert np.array_equal(bits(got_c), bits(got_i))          # (item 3: other rows around the indexed ones change nothing)
    pass_close(got_c, want, S["means"], "%s K=%d" % (case, K))
    # an un-scaled matrix: xs = float32(x / scale)
    scale = np.array([0.037, 0.41], dtype=np.float32)
    raw = (X32 * scale).astype(np.float32)
    Xs = (raw / scale).astype(np.float64)
    lr = H.ref_log_resp(Xs, S)
    pass_close(engine.bgmm_stats_dev(cuda(raw), st, scale).cpu().numpy(), H.ref_sums(Xs, np.exp(lr), lr, S["means"]),
               S["means"])


# ---- 2. the fit from the fixture's labels -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.cases())
def test_fit_from_labels_equals_sklearn(case):
    g = H.case_of(H.golden(), case)
    K = int(g["K"])
    res = engine.bgmm_fit_dev(cuda(g["X"]), ONE, engine.bgmm_fit_params(K, n_init=1), init_labels_t=cuda(g["labels0"]))
    d_par = max(float(np.abs(getattr(res, k) - g[k]).max()) for k in H.PARAM_KEYS)
    d_lb = float(np.abs(res.lower_bounds - g["lower_bounds"][:res.n_iter]).max()) if res.n_iter == int(g["n_iter"]) else np.inf
    print("%s: n_iter %d (sklearn %d)  parameters %.2e (spread %.2e)  bound trace %.2e (spread %.2e)"
          % (case, res.n_iter, int(g["n_iter"]), d_par, float(g["spread_par"]), d_lb, float(g["spread_lb"])))
    assert res.n_iter == int(g["n_iter"]) and res.converged == bool(g["converged"])
    assert d_par <= 100 * float(g["spread_par"])
    assert d_lb <= 100 * float(g["spread_lb"])
    assert res.lower_bound == res.lower_bounds[-1] and res.best_init == 0 and res.n_train == g["X"].shape[0]
    # the state after initialisation only
    init = engine.bgmm_fit_dev(cuda(g["X"]), ONE, engine.bgmm_fit_params(K, n_init=1, max_iter=0),
                               init_labels_t=cuda(g["labels0"]))
    assert init.n_iter == 0 and not init.converged and init.lower_bound == -np.inf
    assert max(float(np.abs(getattr(init, k) - g["init_" + k]).max()) for k in H.PARAM_KEYS) <= 100 * float(g["spread_par"])
    W0 = np.cov(g["X"].astype(np.float64).T).reshape(2, 2)          # (centred sums of n terms: n eps of sqrt(var var))
    assert close(init.cov_prior, W0, 1e-12, scale=np.sqrt(np.outer(np.diag(W0), np.diag(W0))))[1]


# ---- 3. the same bits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["synth_k4", "blobs_k6"])
def test_fit_is_reproducible_to_the_bit(case):
    g = H.case_of(H.golden(), case)
    K = int(g["K"])
    scale = np.array([0.05, 0.6], dtype=np.float32)
    raw = (g["X"] * scale).astype(np.float32)
    p = engine.bgmm_fit_params(K, n_init=1)
    t, lab = cuda(raw), cuda(g["labels0"])
    a = engine.bgmm_fit_dev(t, scale, p, init_labels_t=lab)
    b = engine.bgmm_fit_dev(t, scale, p, init_labels_t=lab)
    assert same_bits(a, b)
    big, idx = embed(raw, 11)
    c = engine.bgmm_fit_dev(cuda(big), scale, p, index_t=cuda(idx), init_labels_t=lab)
    assert same_bits(a, c)
    d = engine.bgmm_fit(big, scale, p, index=idx, init_labels=g["labels0"])          # host arrays, the rows gathered
    assert same_bits(a, d)
    e = engine.bgmm_fit(raw, scale, p, init_labels=g["labels0"])
    assert same_bits(a, e)


# ---- 4. the own initialisation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", [("blobs_k3", 3), ("synth_k4", 4), ("blobs_k8", 8), ("dups_k2", 5)])
def test_kmeans_passes_equal_the_restatement(case, K):
    g = H.case_of(H.golden(), case)
    X32, X = g["X"], g["X"].astype(np.float64)
    centres = bgmm.kmeanspp_centres(X, K, np.random.default_rng(K))
    big, idx = embed(X32, 5)
    t, idx_t = cuda(big), cuda(idx)
    lab_t = torch.full((X.shape[0],), -1, dtype=torch.int32, device="cuda")
    want_labels, want_passes, _ = H.ref_lloyd(X, centres)
    labels = np.full(X.shape[0], -1, dtype=np.int32)
    worst_c = 0.0
    for it in range(1, _lib.BGMM_KMEANS_MAX_ITER + 1):
        sums_t, changed_t = engine.bgmm_kmeans_dev(t, centres, ONE, lab_t, index_t=idx_t)
        new = H.ref_nearest(X, centres)
        assert np.array_equal(lab_t.cpu().numpy(), new)                                   # labels exactly
        assert int(changed_t.item()) == int((new != labels).sum())
        labels = new
        if not int(changed_t.item()):
            break
        sums = sums_t.cpu().numpy()
        assert np.array_equal(sums[:, 0], np.bincount(new, minlength=K).astype(np.float64))
        for k in range(K):
            if sums[k, 0] > 0:
                got = centres[k] + sums[k, 1:3] / sums[k, 0]
                worst_c = max(worst_c, float(np.abs(got - X[new == k].mean(axis=0)).max()))
                centres[k] = centres[k] + (X[new == k] - centres[k]).sum(axis=0) / sums[k, 0]      # the restatement's
    print("%s K=%d: %d passes, centres within %.2e" % (case, K, it, worst_c))
    assert it == want_passes and np.array_equal(labels, want_labels)
    assert worst_c <= 100 * float(g["spread_par"])


def test_own_initialisation_fit_equals_the_restatement_and_names_the_best_run():
    """blobs_k6's points with K = 4 and seed 42: the restatement's five bounds are 15284.67, 15304.16, 15312.72,
    15293.67, 15291.10 -- the third run wins by 8.6, far above any rounding."""
    g = H.case_of(H.golden(), "blobs_k6")
    X32, K = g["X"], 4
    fetch = lambda pos: X32 if pos is None else X32[pos]      # noqa: E731
    centres = bgmm.initial_centres(fetch, X32.shape[0], ONE, K, 42, 5)
    p = engine.bgmm_fit_params(K)
    res = engine.bgmm_fit_dev(cuda(X32), ONE, p, init_centres=centres)
    want = H.ref_own_fit(X32, K, 42, 5)
    print("own initialisation: best run %d (restatement %d), bounds %s, k-means passes %s"
          % (res.best_init, want["run"], res.init_lower_bounds, res.kmeans_iter))
    assert len(res.init_lower_bounds) == 5 and res.best_init == int(np.argmax(res.init_lower_bounds))
    assert res.lower_bound == res.init_lower_bounds.max() and res.n_iter == res.init_n_iter[res.best_init]
    assert res.best_init == want["run"] == 2 and res.n_iter == want["n_iter"] and res.converged == want["converged"]
    assert H.worst({k: getattr(res, k) for k in H.PARAM_KEYS}, want) <= 100 * float(g["spread_par"])
    assert res.kmeans_iter[want["run"]] == H.ref_lloyd(X32.astype(np.float64), centres[want["run"]])[1]
    # ties: five runs from the same centres have the same bound to the bit, and the first is named
    tied = engine.bgmm_fit_dev(cuda(X32), ONE, p, init_centres=np.repeat(centres[1:2], 5, axis=0))
    assert len(set(bits(tied.init_lower_bounds).tolist())) == 1 and tied.best_init == 0
    # a later, better run replaces an earlier one
    two = engine.bgmm_fit_dev(cuda(X32), ONE, engine.bgmm_fit_params(K, n_init=2), init_centres=centres[[0, 2]])
    assert two.best_init == 1 and two.lower_bound == res.lower_bound


# ---- 5. the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_samples,assign_points", [(2000, True), (2000, False), (100000, True), (None, True)])
def test_model_fit_and_fit_dev_agree_bit_for_bit(tmp_path, max_samples, assign_points):
    g = H.case_of(H.golden(), "synth_k2")
    scale = np.array([0.021, 0.33], dtype=np.float32)
    X = (g["X"] * scale).astype(np.float32)
    a = BGMMModel.fit(X, 2, max_samples=max_samples, seed=9, assign_points=assign_points)
    b = BGMMModel.fit_dev(cuda(X), 2, max_samples=max_samples, seed=9, assign_points=assign_points)
    for k in ("weights", "means", "covariances"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k)))
    assert np.array_equal(a.scale, b.scale) and a.scale.dtype == np.float32
    assert (a.within_label, a.between_label) == (b.within_label, b.between_label) and bytes(a.model) == bytes(b.model)
    for k in ("n_iter", "converged", "lower_bound", "n_train", "init", "best_init"):
        assert a.fit_info[k] == b.fit_info[k]
    assert np.array_equal(bits(a.fit_info["lower_bounds"]), bits(b.fit_info["lower_bounds"]))
    n_train = X.shape[0] if (max_samples is None or max_samples >= X.shape[0]) else max_samples
    assert a.fit_info["n_train"] == n_train and a.fit_info["init"] == "kmeans++"
    assert np.array_equal(a.labels, b.labels.cpu().numpy()) and a.labels.dtype == np.int64
    idx = None if n_train == X.shape[0] else DBSCANModel.subsample_index(X.shape[0], max_samples, 9)
    rows = X if (assign_points or idx is None) else X[idx]
    assert np.array_equal(a.scale, np.amax(X if idx is None else X[idx], axis=0))
    # labels are the assignment of the saved arrays
    loaded = BGMMModel.from_npz(a.save(tmp_path / "fit"))
    plain = BGMMModel(a.weights, a.means, a.covariances, a.scale, a.within_label, a.between_label)
    assert np.array_equal(a.labels, plain.assign(rows)) and np.array_equal(a.labels, loaded.assign(rows))
    assert a.within_label == bgmm.findWithinLabel(a.means, a.labels)
    assert a.between_label == bgmm.findBetweenLabel_bgmm(a.means, a.labels)
    # given labels: one run
    lab = (np.arange(n_train) % 2).astype(np.int32)
    c = BGMMModel.fit(X, 2, max_samples=max_samples, seed=9, init_labels=lab)
    d = BGMMModel.fit_dev(cuda(X), 2, max_samples=max_samples, seed=9, init_labels=lab)
    assert c.fit_info["init"] == "labels" and len(c.fit_info["init_lower_bounds"]) == 1
    assert np.array_equal(bits(c.means), bits(d.means)) and np.array_equal(bits(c.covariances), bits(d.covariances))


def test_device_argument_errors():
    X = np.abs(np.random.default_rng(0).normal(0.3, 0.1, (500, 2))).astype(np.float32)
    lab = (np.arange(500) % 3).astype(np.int32)
    p = engine.bgmm_fit_params(3, n_init=1)
    bad = X.copy()
    bad[321, 1] = np.nan
    bad[400, 0] = np.inf
    with pytest.raises(ValueError, match="training row 321 is not finite"):
        engine.bgmm_fit_dev(cuda(bad), ONE, p, init_labels_t=cuda(lab))
    with pytest.raises(ValueError, match="training row 2 is not finite"):
        engine.bgmm_fit_dev(cuda(bad), ONE, p, index_t=cuda(np.array([5, 6, 400, 321, 8], dtype=np.int64)),
                            init_labels_t=cuda(lab[:5]))
    wrong = lab.copy()
    wrong[77] = 3
    with pytest.raises(ValueError, match=r"label of training row 77 is outside \[0, 3\)"):
        engine.bgmm_fit_dev(cuda(X), ONE, p, init_labels_t=cuda(wrong))
    with pytest.raises(ValueError, match="index entry 1 is outside the matrix of 500 rows"):
        engine.bgmm_fit_dev(cuda(X), ONE, p, index_t=cuda(np.array([0, 500, 3], dtype=np.int64)), init_labels_t=cuda(lab[:3]))
    with pytest.raises(ValueError, match="fewer training rows"):
        engine.bgmm_fit_dev(cuda(X[:2]), ONE, p, init_labels_t=cuda(lab[:2]))
    with pytest.raises(ValueError, match="scale must be positive"):
        engine.bgmm_fit_dev(cuda(X), (0.0, 1.0), p, init_labels_t=cuda(lab))
    # every row the same point (the origin): the covariance prior and every component's covariance are zero
    same = np.zeros((64, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="lost positive-definiteness"):
        engine.bgmm_fit_dev(cuda(same), ONE, engine.bgmm_fit_params(1, n_init=1, reg_covar=0.0),
                            init_labels_t=cuda(np.zeros(64, dtype=np.int32)))


# ---- 6. the whole matrix -----------------------------------------------------------------------------------------------
def test_whole_matrix_fit():
    """49 995 000 rows, no subsample.  Against the restatement on the host for two iterations, from the labels of one
    k-means pass.  Bars (no recorded spread at this size): parameters 1e-10 max(1, |value|), bound 1e-11 |bound| --
    tree-shaped sums of n terms lose about log2(n) eps = 6e-15 of their value, the three lgamma of betaln at a, b of
    5e7 lose 3 eps 8.4e8 = 6e-7 against a bound of 1e8 and more, and exp / log differ by an ulp or two per term: three
    orders in hand."""
    from poppunk_amd import synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    db = engine.SketchDB(synth.make_sketches_device(10000, kmers, device="cuda:0"), 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    n = dist_t.shape[0]
    assert n == 49_995_000
    a = BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    b = BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    print("whole matrix: %s" % {k: a.fit_info[k] for k in ("n_iter", "converged", "lower_bound", "n_train", "best_init")})
    assert a.fit_info["n_train"] == n and np.isfinite(a.fit_info["lower_bound"]) and a.fit_info["n_iter"] >= 1
    for k in ("weights", "means", "covariances"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k)))
    assert np.array_equal(bits(a.fit_info["lower_bounds"]), bits(b.fit_info["lower_bounds"]))
    assert torch.equal(a.labels, b.labels) and a.labels.shape[0] == n
    assert abs(a.weights.sum() - 1.0) < 1e-12
    # two iterations against the host
    scale = a.scale
    X = (dist_t.cpu().numpy() / scale).astype(np.float64)
    centres = np.array([[0.1, 0.1], [0.7, 0.7]])
    lab_t = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    engine.bgmm_kmeans_dev(dist_t, centres, scale, lab_t)
    labels = lab_t.cpu().numpy()
    assert np.array_equal(labels, H.ref_nearest(X, centres))
    got = engine.bgmm_fit_dev(dist_t, scale, engine.bgmm_fit_params(2, n_init=1, max_iter=2), init_labels_t=lab_t)
    want = H.ref_fit(X, labels, 2, max_iter=2)
    assert got.n_iter == 2
    d_par = max(close(getattr(got, k), want[k], scale=np.maximum(1.0, np.abs(want[k])))[0] for k in H.PARAM_KEYS)
    d_lb = float((np.abs(got.lower_bounds - want["lower_bounds"]) / np.abs(want["lower_bounds"])).max())
    print("whole matrix, two iterations: parameters %.2e, bound (relative) %.2e" % (d_par, d_lb))
    assert d_par <= 1e-10 and d_lb <= 1e-11


# ---- 7. end to end ------------------------------------------------------------------------------------------------------
def test_end_to_end_clusters_equal_the_sklearn_models(golden_dir):
    """The database bgmm_assign.npz's k2 model (an sklearn fit) was fitted on: the clusters of this fit's edge list are
    the partition that model's edge list gives (confirmed for the restatement with the own initialisation on the CPU)."""
    from poppunk_amd import distfile, synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(240, kmers, cluster_size=20, seed=7)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    with np.load(os.path.join(golden_dir, "bgmm_assign.npz"), allow_pickle=False) as z:
        theirs = BGMMModel(z["k2_weights"], z["k2_means"], z["k2_covariances"], z["k2_scale"], z["k2_within"].item(),
                           z["k2_between"].item())
    ours = BGMMModel.fit_dev(dist_t, 2, seed=42)
    parts = []
    for m in (ours, theirs):
        edges = engine.bgmm_edges_dev(dist_t, m.model).cpu().numpy()
        n_clusters, labels = distfile.clusters_from_edges(240, edges)
        parts.append((n_clusters, labels, len(edges)))
    print("end to end: %d / %d within-strain pairs, %d / %d clusters, fit %s"
          % (parts[0][2], parts[1][2], parts[0][0], parts[1][0], {k: ours.fit_info[k] for k in ("n_iter", "best_init")}))
    assert parts[0][0] == parts[1][0] == len(set(zip(parts[0][1].tolist(), parts[1][1].tolist())))
