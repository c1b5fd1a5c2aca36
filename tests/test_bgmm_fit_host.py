"""CPU tests of the BGMM fit (include/ppk.h "BGMM fit"): a numpy restatement of the definition against
sklearn's recorded fits (tests/golden/bgmm_fit.npz), the host-only M-step and digamma of libppk_hip.so against the
restatement and scipy, the within / between label rules, save -> load, and the argument errors of the ABI.

The restatement (ref_*) is what the GPU suite (tests/test_gpu_bgmm_fit.py) compares the device with, and what
tests/golden/make_golden_bgmm_fit.py checks against sklearn before it writes a case.  ref_sums_exact (the sums of one
pass with math.fsum, and the scale each is compared on) and the seeded inputs of tests/test_gpu_bgmm_fit_shapes.py
live here too, with the CPU tests of both."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
from scipy.special import betaln, digamma, gammaln

from poppunk_amd import _lib, bgmm, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bgmm_fit.npz")
EPS = np.finfo(np.float64).eps
PRIORS = dict(wcp=0.1, mpp=0.1, m0=np.zeros(2), dof0=2.0, reg=1e-6)      # fit2dMultiGaussian + sklearn's defaults
PARAM_KEYS = ("weights", "means", "covariances", "weight_concentration", "mean_precision", "degrees_of_freedom")


# ---- the definition, in numpy -----------------------------------------------------------------------------------------
def ref_stats(X, resp, reg=PRIORS["reg"]):
    """nk, xk, sk of responsibilities [n, K] (two passes: centred on xk)."""
    nk = resp.sum(axis=0) + 10 * EPS
    xk = resp.T @ X / nk[:, None]
    sk = np.empty((nk.size, 2, 2))
    for k in range(nk.size):
        d = X - xk[k]
        sk[k] = (resp[:, k] * d.T) @ d / nk[k]
        sk[k].flat[::3] += reg
    return nk, xk, sk


def ref_mstep(nk, xk, sk, W0, P=PRIORS):
    a = 1.0 + nk
    b = P["wcp"] + np.hstack((np.cumsum(nk[::-1])[-2::-1], 0))
    beta = P["mpp"] + nk
    means = (P["mpp"] * P["m0"] + nk[:, None] * xk) / beta[:, None]
    dof = P["dof0"] + nk
    cov = np.empty_like(sk)
    for k in range(nk.size):
        d = xk[k] - P["m0"]
        cov[k] = W0 + nk[k] * (sk[k] + P["mpp"] / beta[k] * np.outer(d, d))
    cov /= dof[:, None, None]
    return dict(a=a, b=b, beta=beta, means=means, dof=dof, cov=cov)


def ref_chol(S):
    return np.stack([np.linalg.cholesky(c) for c in S["cov"]])


def ref_weighted_log_prob(X, S):
    """The E-step's weighted log-probabilities w [n, K]."""
    K = S["a"].size
    ds = digamma(S["a"] + S["b"])
    log_w = digamma(S["a"]) - ds + np.hstack((0, np.cumsum(digamma(S["b"]) - ds)[:-1]))
    lp = np.empty((X.shape[0], K))
    for k, L in enumerate(ref_chol(S)):
        Pc = np.linalg.inv(L).T                                  # the precision's Cholesky factor, upper
        y = X @ Pc - S["means"][k] @ Pc
        lp[:, k] = -0.5 * (2 * np.log(2 * np.pi) + (y * y).sum(axis=1)) + np.log(np.diag(Pc)).sum()
    lp -= 0.5 * 2 * np.log(S["dof"])
    log_lambda = 2 * np.log(2.0) + digamma(0.5 * S["dof"]) + digamma(0.5 * (S["dof"] - 1))
    return lp + 0.5 * (log_lambda - 2 / S["beta"]) + log_w


def ref_logsumexp(w):
    """scipy's logsumexp over the components: max + log sum exp(w - max)."""
    m = w.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(w - m).sum(axis=1))


def ref_log_resp(X, S):
    """The E-step: log responsibilities [n, K]."""
    w = ref_weighted_log_prob(X, S)
    return w - ref_logsumexp(w)[:, None]


def ref_bound(log_resp, S):
    L = ref_chol(S)
    dof = S["dof"]
    ldpc = -np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1) - 0.5 * 2 * np.log(dof)
    lwn = -(dof * ldpc + dof * 2 * 0.5 * np.log(2.0) + gammaln(0.5 * dof) + gammaln(0.5 * (dof - 1)))
    return (-(np.exp(log_resp) * log_resp).sum() - lwn.sum() + betaln(S["a"], S["b"]).sum()
            - 0.5 * 2 * np.log(S["beta"]).sum())


def ref_weights(S):
    ws = S["a"] + S["b"]
    w = S["a"] / ws * np.hstack((1, np.cumprod((S["b"] / ws)[:-1])))
    return w / w.sum()


def ref_params(S):
    return {"weights": ref_weights(S), "means": S["means"], "covariances": S["cov"],
            "weight_concentration": np.stack([S["a"], S["b"]]), "mean_precision": S["beta"],
            "degrees_of_freedom": S["dof"]}


def one_hot(labels, K):
    resp = np.zeros((labels.shape[0], K))
    resp[np.arange(labels.shape[0]), labels] = 1
    return resp


def ref_fit(X, labels, K, tol=1e-3, max_iter=100):
    """The fit from initial labels on float64 rows: the parameters, the run's trace and the state after
    initialisation (`init`) and after the first iteration (`first`)."""
    W0 = np.atleast_2d(np.cov(X.T))
    S = ref_mstep(*ref_stats(X, one_hot(labels, K)), W0)
    out = {"init": S, "first": None, "W0": W0}
    lb, bounds, it, converged = -np.inf, [], 0, False
    for it in range(1, max_iter + 1):
        prev = lb
        lr = ref_log_resp(X, S)
        S = ref_mstep(*ref_stats(X, np.exp(lr)), W0)
        lb = ref_bound(lr, S)
        bounds.append(lb)
        if it == 1:
            out["first"] = S
        if abs(lb - prev) < tol:
            converged = True
            break
    out.update(ref_params(S), state=S, n_iter=it, converged=converged, lower_bound=lb, lower_bounds=np.array(bounds))
    return out


def ref_sums(X, resp, log_resp, pivot):
    """What one device pass returns: per component S r, S r d (2), S r d d^T (3), S r log r about pivot [K, 2]."""
    K = resp.shape[1]
    out = np.zeros((K, 7))
    for k in range(K):
        d, r = X - pivot[k], resp[:, k]
        out[k] = [r.sum(), (r * d[:, 0]).sum(), (r * d[:, 1]).sum(), (r * d[:, 0] * d[:, 0]).sum(),
                  (r * d[:, 0] * d[:, 1]).sum(), (r * d[:, 1] * d[:, 1]).sum(),
                  0.0 if log_resp is None else (r * log_resp[:, k]).sum()]
    return out


def ref_sums_exact(X64, S, pivot, counts=None):
    """One device pass with no summation error of its own: (sums [K, 7], scales [K, 7]).

    X64: the scaled rows xs = float32(x / scale) widened to float64.  S: a variational state (the E-step's
    responsibilities) or an integer label per row (the one-hot passes: w = lse = 0).  counts[i]: how often row i occurs
    (its term is multiplied by it), so n rows that repeat a block cyclically cost the block's terms only.  The terms
    are float64 numpy, as ref_log_resp and ref_sums compute them; each sum is math.fsum's, exactly rounded.

    scales[k, s] = S_i |term_iks| (1 + |w_ik| + |lse_i|), the seventh sum's term being r (1 + |log r|): log r = w - lse
    carries an absolute error of a few eps (|w| + |lse|) (ppk_bgmm_lpr's multiply-add chain, device exp / log an ulp
    or two from libm), r = exp(log r) carries that as a relative error, and the device's sum of the terms (at most 9
    serial additions per lane below the grid's cap, then fixed trees) adds about 30 eps S |term|."""
    pivot = np.asarray(pivot, dtype=np.float64)
    K = pivot.shape[0]
    if isinstance(S, dict):
        w = ref_weighted_log_prob(X64, S)
        lse = ref_logsumexp(w)
        lr = w - lse[:, None]
        r = np.exp(lr)
        amp = 1.0 + np.abs(w) + np.abs(lse)[:, None]
    else:
        r = one_hot(np.asarray(S), K)
        lr = np.zeros_like(r)
        amp = np.ones_like(r)
    c = np.ones(X64.shape[0]) if counts is None else np.asarray(counts, dtype=np.float64)
    sums, scales = np.zeros((K, 7)), np.zeros((K, 7))
    for k in range(K):
        d, rk = X64 - pivot[k], r[:, k]
        terms = [rk, rk * d[:, 0], rk * d[:, 1], rk * d[:, 0] * d[:, 0], rk * d[:, 0] * d[:, 1], rk * d[:, 1] * d[:, 1],
                 rk * lr[:, k]]
        sizes = [np.abs(t) for t in terms[:6]] + [rk * (1.0 + np.abs(lr[:, k]))]
        for s in range(7):
            sums[k, s] = math.fsum((c * terms[s]).tolist())
            scales[k, s] = math.fsum((c * sizes[s] * amp[:, k]).tolist())
    return sums, scales


def ref_nearest(X, centres):
    """Labels under (d2, index of centre), d2 = dx dx + dy dy."""
    d2 = np.stack([(X[:, 0] - c[0]) * (X[:, 0] - c[0]) + (X[:, 1] - c[1]) * (X[:, 1] - c[1]) for c in centres], axis=1)
    return np.argmin(d2, axis=1).astype(np.int32)


def ref_lloyd(X, centres, max_iter=_lib.BGMM_KMEANS_MAX_ITER):
    """The own initialisation: (labels of the last pass, passes made, centres the last pass read)."""
    centres = np.array(centres, dtype=np.float64)
    labels = np.full(X.shape[0], -1, dtype=np.int32)
    for it in range(1, max_iter + 1):
        new = ref_nearest(X, centres)
        changed = int((new != labels).sum())
        labels = new
        if not changed:
            break
        for k in range(centres.shape[0]):
            if np.any(labels == k):
                centres[k] = centres[k] + (X[labels == k] - centres[k]).sum(axis=0) / np.count_nonzero(labels == k)
    return labels, it, centres


def ref_own_fit(X32_scaled, K, seed, n_init, max_iter=100):
    """The whole own-initialisation fit on scaled float32 rows: best of n_init, the first on ties."""
    X = X32_scaled.astype(np.float64)
    best = None
    for r in range(n_init):
        rng = np.random.default_rng(seed + r)
        pos = bgmm.seeding_positions(X.shape[0], rng)
        c0 = bgmm.kmeanspp_centres(X if pos is None else X[pos], K, rng)
        labels, _, _ = ref_lloyd(X, c0)
        f = ref_fit(X, labels, K, max_iter=max_iter)
        f["run"], f["labels0"] = r, labels
        if best is None or f["lower_bound"] > best["lower_bound"]:
            best = f
    return best


def ref_assign(X, weights, means, covariances):
    """BGMMFit.assign's labels (PopPUNK/bgmm.py:100-176) on scaled float64 rows."""
    lpr = np.empty((X.shape[0], len(weights)))
    for k in range(len(weights)):
        L = np.linalg.cholesky(covariances[k])
        z = np.linalg.solve(L, (X - means[k]).T).T
        lpr[:, k] = np.log(weights[k]) - 0.5 * ((z * z).sum(axis=1) + 2 * np.log(2 * np.pi) + 2 * np.log(np.diag(L)).sum())
    return lpr.argmax(axis=1)


# ---- helpers -------------------------------------------------------------------------------------------------------
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cases():
    if not os.path.exists(GOLDEN):          # (the generator imports this module before the fixture exists)
        return []
    with np.load(GOLDEN, allow_pickle=False) as z:
        return [str(c) for c in z["cases"]]


def case_of(g, c):
    return {k[len(c) + 1:]: v for k, v in g.items() if k.startswith(c + "_")}


def worst(got, want):
    """Largest absolute difference over the fitted parameters."""
    return max(float(np.abs(np.asarray(got[k]) - np.asarray(want[k])).max()) for k in PARAM_KEYS)


def lib_mstep(K, sums, pivot, W0, **overrides):
    """ppk_bgmm_mstep -> (dict of state arrays, bound)."""
    params = engine.bgmm_fit_params(K, **overrides)
    state, lb = _lib.BgmmState(), C.c_double()
    f64p = C.POINTER(C.c_double)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (sums, pivot, W0)]
    rc = _lib.lib().ppk_bgmm_mstep(C.byref(params), *[a.ctypes.data_as(f64p) for a in arrs], C.byref(state), C.byref(lb))
    if rc == _lib.ERR_ARG:
        raise ValueError(_lib.last_error())
    _lib.check(rc, "ppk_bgmm_mstep")
    return bgmm.state_arrays(state), lb.value, state


def state_from_ref(S, K):
    """The `_lib.BgmmState` of a restatement state: through ppk_bgmm_mstep would need sums, so it is filled directly
    (what the E-step reads: lin, log_const, means)."""
    st = _lib.BgmmState()
    st.K = K
    ds = digamma(S["a"] + S["b"])
    log_w = digamma(S["a"]) - ds + np.hstack((0, np.cumsum(digamma(S["b"]) - ds)[:-1]))
    for k, L in enumerate(ref_chol(S)):
        i0, i1 = 1.0 / L[0, 0], 1.0 / L[1, 1]
        st.means[k][0], st.means[k][1] = S["means"][k]
        for j, v in enumerate((i0, -S["means"][k][0] * i0, i1, -L[1, 0] * i1, -S["means"][k][1] * i1)):
            st.lin[k][j] = v
        log_lambda = 2 * np.log(2.0) + digamma(0.5 * S["dof"][k]) + digamma(0.5 * (S["dof"][k] - 1))
        st.log_const[k] = ((-0.5 * 2 * np.log(2 * np.pi) + np.log(i0) + np.log(i1)) - 0.5 * 2 * np.log(S["dof"][k])
                           + 0.5 * (log_lambda - 2 / S["beta"][k]) + log_w[k])
    return st


# ---- inputs of the shape tests (tests/test_gpu_bgmm_fit_shapes.py): one generator, its conditions asserted below ---------
SHAPE_BLOCK = 4099                                          # rows of the block; larger n repeats it cyclically
SHAPE_SCALE = np.array([0.037, 0.41], dtype=np.float32)
SHAPE_KS = tuple(range(1, _lib.BGMM_MAX_K + 1))
SHAPE_OUTLIERS, SHAPE_DUPLICATES = 41, 82                   # 1 % and 2 % of the block
PLANTED = (1000.0, -1000.0)                                 # a centre no row is nearest to


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def shape_block():
    """(raw float32 [4099, 2], xs = float32(raw / scale) as float64, positions of the outliers, of the duplicates and of
    the rows they copy).  The rows lie around 16 centres on a 4 x 4 grid in [0, 1]^2 (sigma 0.02, a tenth of the
    spacing) in scaled units; the outliers 40 to 60 units from (0.5, 0.5), where the components that hold no outlier
    underflow to a responsibility of 0."""
    rng = np.random.default_rng(20261020)
    n = SHAPE_BLOCK
    g = (np.arange(4) + 0.5) / 4
    centres = np.array([(a, b) for a in g for b in g])
    X = centres[rng.integers(0, 16, n)] + rng.normal(0.0, 0.02, (n, 2))
    pos = rng.permutation(n)
    out, dup = pos[:SHAPE_OUTLIERS], pos[SHAPE_OUTLIERS:SHAPE_OUTLIERS + SHAPE_DUPLICATES]
    src = pos[SHAPE_OUTLIERS + SHAPE_DUPLICATES:SHAPE_OUTLIERS + 2 * SHAPE_DUPLICATES]
    angle = rng.uniform(0.0, 2 * np.pi, out.size)
    X[out] = 0.5 + 40.0 * rng.uniform(1.0, 1.5, (out.size, 1)) * np.stack([np.cos(angle), np.sin(angle)], axis=1)
    X[dup] = X[src]
    raw = (X * SHAPE_SCALE).astype(np.float32)
    xs = (raw / SHAPE_SCALE).astype(np.float64)
    return tuple(_frozen(a) for a in (raw, xs, out, dup, src))


def shape_rows(n):
    """Positions in the block of the n rows of a case: the block repeated cyclically."""
    return np.arange(n) % SHAPE_BLOCK


def shape_counts(n):
    """How often each row of the block occurs among shape_rows(n)."""
    return n // SHAPE_BLOCK + (np.arange(SHAPE_BLOCK) < n % SHAPE_BLOCK)


def shape_labels(n, K):
    return (np.arange(n) * 7 % K).astype(np.int32)


@functools.lru_cache(maxsize=None)
def shape_state(K):
    """The K-component state every row count uses: the restatement's first iteration on the block from arbitrary labels
    (only parameters; K = 7 and 14 leave components with next to no responsibility, which the scale carries)."""
    return ref_fit(shape_block()[1], shape_labels(SHAPE_BLOCK, K), K, max_iter=1)["first"]


@functools.lru_cache(maxsize=None)
def shape_centres(K, n):
    """Two sets of K centres for the first n rows of the block: k-means++ centres of its inliers with PLANTED inserted
    at K // 2 (K = 1: the one drawn centre), and what one Lloyd step makes of them (an emptied centre keeps its
    place)."""
    X = shape_block()[1][:n]
    inliers = X[np.abs(X - 0.5).max(axis=1) < 0.5]              # (drawn from every row, most centres would be outliers)
    rng = np.random.default_rng(1000 * K + n)
    if K == 1:
        first = bgmm.kmeanspp_centres(inliers, 1, rng)
    else:
        first = np.insert(bgmm.kmeanspp_centres(inliers, K - 1, rng), K // 2, PLANTED, axis=0)
    second = first.copy()
    labels = ref_nearest(X, first)
    for k in range(K):
        if np.any(labels == k):
            second[k] = first[k] + (X[labels == k] - first[k]).sum(axis=0) / np.count_nonzero(labels == k)
    return _frozen(first), _frozen(second)


@functools.lru_cache(maxsize=None)
def tied_set():
    """(rows float32 [n, 2] at scale (1, 1), centres [9, 2], a second set of 5 centres): every coordinate a multiple of
    2^-6 below 4 in size, so every d2 and every sum of the pass is exact in double, in any order.  The rows are the
    1/16 grid over [-0.5, 2.5]^2 (2 401 rows, two workgroups) and one more.  Centres 0 to 3 are the unit square's corners
    (its centre ties four, its edges' midpoints two); (1.375, 0.5) ties centres 1, 3 and 4 and (1.5, 0.75) centres 3
    and 4, across the edge between the first four components and the next; centres 5 and 6 are the same point.  The
    second set repeats centre 1 as 2 and centre 3 as 4."""
    t = np.arange(-8, 41) / 16.0
    rows = np.array([(x, y) for x in t for y in t] + [(1.375, 0.5)], dtype=np.float32)
    nine = np.array([(0, 0), (1, 0), (0, 1), (1, 1), (2, 0.5), (2, 2), (2, 2), (0, 2), (1, 2)], dtype=np.float64)
    five = nine[[0, 1, 1, 3, 3]]
    return _frozen(rows), _frozen(nine), _frozen(five)


def nearest_d2(X, centres):
    return np.stack([(X[:, 0] - c[0]) * (X[:, 0] - c[0]) + (X[:, 1] - c[1]) * (X[:, 1] - c[1]) for c in centres], axis=1)


# ---- tests ---------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_must():
    g = golden()
    cs = cases()
    Ks = sorted(int(g[c + "_K"]) for c in cs)
    assert Ks[0] == 1 and Ks[-1] >= 6
    n_iter = {c: int(g[c + "_n_iter"]) for c in cs}
    assert any(v <= 30 and bool(g[c + "_converged"]) for c, v in n_iter.items())
    assert any(v == 100 and not bool(g[c + "_converged"]) for c, v in n_iter.items())
    assert any(g[c + "_weights"].min() < 5e-3 for c in cs)                      # a component the prior left near-empty
    assert any(bool(g[c + "_has_duplicates"]) for c in cs)
    for c in cs:
        assert float(g[c + "_stop_margin"]) >= 1e-6
        assert g[c + "_X"].dtype == np.float32 and g[c + "_labels0"].dtype == np.int32


@pytest.mark.parametrize("case", cases())
def test_restatement_equals_sklearn(case):
    g = case_of(golden(), case)
    K = int(g["K"])
    f = ref_fit(g["X"].astype(np.float64), g["labels0"], K)
    par, lb = 10 * float(g["spread_par"]), 10 * float(g["spread_lb"])
    assert f["n_iter"] == int(g["n_iter"]) and f["converged"] == bool(g["converged"])
    assert worst(f, g) <= par
    assert np.abs(f["lower_bounds"] - g["lower_bounds"]).max() <= lb
    assert worst(ref_params(f["init"]), {k: g["init_" + k] for k in PARAM_KEYS}) <= par


@pytest.mark.parametrize("case", cases())
def test_host_mstep_gives_the_state_after_initialisation_and_after_the_first_iteration(case):
    g = case_of(golden(), case)
    K = int(g["K"])
    X = g["X"].astype(np.float64)
    f = ref_fit(X, g["labels0"], K, max_iter=1)
    par, lb_bar = 10 * float(g["spread_par"]), 10 * float(g["spread_lb"])
    # initialisation: one-hot responsibilities, about the component means (as the library's second pass takes them)
    resp = one_hot(g["labels0"], K)
    _, xk, _ = ref_stats(X, resp)
    got, _, _ = lib_mstep(K, ref_sums(X, resp, None, xk), xk, f["W0"])
    assert worst(got, {k: g["init_" + k] for k in PARAM_KEYS}) <= par
    # first iteration: the E-step of the initial state, sums about its means
    lr = ref_log_resp(X, f["init"])
    got, lb, _ = lib_mstep(K, ref_sums(X, np.exp(lr), lr, f["init"]["means"]), f["init"]["means"], f["W0"])
    assert worst(got, ref_params(f["first"])) <= par
    assert abs(lb - float(g["lower_bounds"][0])) <= lb_bar
    if int(g["n_iter"]) == 1:
        assert worst(got, g) <= par


def test_mstep_state_feeds_the_e_step_it_describes():
    """lin / log_const of ppk_bgmm_mstep reproduce the restatement's weighted log-probabilities."""
    g = case_of(golden(), cases()[0])
    K = int(g["K"])
    X = g["X"].astype(np.float64)
    f = ref_fit(X, g["labels0"], K, max_iter=1)
    lr = ref_log_resp(X, f["init"])
    got, _, _ = lib_mstep(K, ref_sums(X, np.exp(lr), lr, f["init"]["means"]), f["init"]["means"], f["W0"])
    z0 = X[:, :1] * got["lin"][:, 0] + got["lin"][:, 1]
    z1 = X[:, 1:] * got["lin"][:, 2] + (z0 * got["lin"][:, 3] + got["lin"][:, 4])
    w = got["log_const"] - 0.5 * (z0 * z0 + z1 * z1)
    mine = w - (w.max(axis=1) + np.log(np.exp(w - w.max(axis=1, keepdims=True)).sum(axis=1)))[:, None]
    assert np.abs(mine - ref_log_resp(X, f["first"])).max() <= 1e-9


def test_digamma_against_scipy():
    """Bar: 16 eps max(1, |psi|).  The recurrence makes at most 10 subtractions, each rounding the running value (at
    most max(|psi|, psi(10) = 2.25) in size) by half an ulp, and the logarithm and the series add an ulp each: 7 ulp
    of max(1, |psi|) at worst, 16 eps with a factor of two in hand.  Measured on this grid: 5 eps.  (An error relative
    to psi itself has no bound near its root at 1.4616.)"""
    lib = _lib.lib()
    x = np.concatenate([np.geomspace(0.1, 1e8, 20001), np.linspace(0.1, 30.0, 5001)])
    got = np.array([lib.ppk_bgmm_digamma(float(v)) for v in x])
    want = digamma(x)
    assert (np.abs(got - want) / (EPS * np.maximum(1.0, np.abs(want)))).max() <= 16
    assert np.isnan(lib.ppk_bgmm_digamma(0.0)) and np.isnan(lib.ppk_bgmm_digamma(-1.5))


def test_within_and_between_labels_follow_the_reference(golden_dir):
    with np.load(os.path.join(golden_dir, "bgmm_assign.npz"), allow_pickle=False) as z:
        for case in ("k2", "k4"):
            means, y = z[case + "_means"], z[case + "_labels"]
            # (the committed labels are those of a sample of the fit's rows plus probes: the rules only ask which labels occur and how often)
            own = y[:3000]
            assert bgmm.findWithinLabel(means, own) == int(z[case + "_within"])
            assert bgmm.findBetweenLabel_bgmm(means, own) == int(z[case + "_between"])
    means = np.array([[0.5, 0.5], [0.1, 0.1], [0.1, 0.1], [0.9, 0.9]])
    assert bgmm.findWithinLabel(means, np.array([0, 2, 2, 3, 3])) == 2          # label 1 is unused
    assert bgmm.findWithinLabel(means, np.array([0, 1, 2, 3])) == 1             # the first on ties
    assert bgmm.findBetweenLabel_bgmm(means, np.array([0, 2, 2, 3, 3])) == 2    # the first on ties
    assert bgmm.findWithinLabel(means, np.array([0, 1, 2, 3]), rank=1) == 2


def test_save_writes_the_reference_keys_and_loads_back(tmp_path):
    from poppunk_amd.models import BGMMModel
    g = case_of(golden(), cases()[0])
    K = int(g["K"])
    m = BGMMModel(g["weights"], g["means"], g["covariances"], np.array([0.02, 0.4], dtype=np.float32), K - 1, 0)
    path = m.save(tmp_path / "strain_db")
    assert path == str(tmp_path / "strain_db" / "strain_db_fit.npz")
    assert sorted(os.listdir(tmp_path / "strain_db")) == ["strain_db_fit.npz"]          # no _fit.pkl
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"weights", "means", "covariances", "within", "between", "scale"}
        assert z["within"].item() == K - 1 and z["between"].item() == 0 and z["scale"].dtype == np.float32
    back = BGMMModel.from_npz(path)
    for k in ("weights", "means", "covariances", "scale"):
        assert np.array_equal(getattr(back, k), getattr(m, k))
    assert (back.within_label, back.between_label) == (m.within_label, m.between_label)
    assert bytes(back.model) == bytes(m.model)
    # a model fitted here also stores its variational state under ppk_* keys
    f = ref_fit(g["X"].astype(np.float64), g["labels0"], K, max_iter=1)
    lr = ref_log_resp(g["X"].astype(np.float64), f["init"])
    _, _, state = lib_mstep(K, ref_sums(g["X"].astype(np.float64), np.exp(lr), lr, f["init"]["means"]),
                            f["init"]["means"], f["W0"])
    res = _lib.BgmmFitResult()
    res.state, res.n_iter, res.converged, res.n_init_run, res.n_train, res.lower_bound = state, 1, 0, 1, 7, -3.5
    m.fit_result, m.seed = bgmm.FitResult(res), 42
    with np.load(m.save(tmp_path / "again"), allow_pickle=False) as z:
        assert {"weights", "means", "covariances", "within", "between", "scale"} <= set(z.files)
        assert all(k.startswith("ppk_") for k in set(z.files) - {"weights", "means", "covariances", "within", "between", "scale"})
        assert z["ppk_n_iter"].item() == 1 and z["ppk_seed"].item() == 42 and z["ppk_lower_bound"].item() == -3.5
        assert z["ppk_weight_concentration"].shape == (2, K) and z["ppk_degrees_of_freedom"].shape == (K,)
    BGMMModel.from_npz(str(tmp_path / "again" / "again_fit.npz"))


def test_struct_sizes_and_symbols_through_the_abi():
    import re
    src = open(os.path.join(ROOT, "include", "ppk.h")).read()
    assert 'section "BGMM fit"' in src and "BGMM fit: PopPUNK's default" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for n in ("ppk_bgmm_fit_params_default", "ppk_bgmm_fit_struct_sizes", "ppk_bgmm_digamma", "ppk_bgmm_mstep", "ppk_bgmm_stats_dev",
              "ppk_bgmm_kmeans_dev", "ppk_bgmm_fit_dev", "ppk_bgmm_fit"):
        assert re.search(r"\b%s\s*\(" % n, code) and n in _lib.SIGNATURES and hasattr(lib, n)
    for macro, value in (("PPK_BGMM_FIT_STATS", _lib.BGMM_FIT_STATS), ("PPK_BGMM_FIT_MAX_ITER", _lib.BGMM_FIT_MAX_ITER),
                         ("PPK_BGMM_FIT_MAX_INIT", _lib.BGMM_FIT_MAX_INIT),
                         ("PPK_BGMM_KMEANS_MAX_ITER", _lib.BGMM_KMEANS_MAX_ITER), ("PPK_BGMM_MAX_K", _lib.BGMM_MAX_K)):
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == value
    # the layouts the header declares, field by field (all members are 4- or 8-byte scalars, 8-byte aligned groups)
    K, I, R = _lib.BGMM_MAX_K, _lib.BGMM_FIT_MAX_ITER, _lib.BGMM_FIT_MAX_INIT
    assert C.sizeof(_lib.BgmmFitParams) == 4 * 4 + 8 * 7
    assert C.sizeof(_lib.BgmmState) == 8 + 8 * K * (2 + 1 + 2 + 1 + 4 + 3 + 1 + 5 + 1)
    assert C.sizeof(_lib.BgmmFitResult) == C.sizeof(_lib.BgmmState) + 4 * 4 + 8 + 8 + 8 * 4 + 8 * 2 + 8 * R + 4 * R * 2 + 8 * I
    sizes = (C.c_size_t * 3)()
    assert lib.ppk_bgmm_fit_struct_sizes(sizes) == _lib.OK
    assert list(sizes) == [C.sizeof(_lib.BgmmFitParams), C.sizeof(_lib.BgmmState), C.sizeof(_lib.BgmmFitResult)]
    # the library fills the structs where ctypes reads them
    p = engine.bgmm_fit_params(3)
    assert (p.K, p.max_iter, p.n_init) == (3, 100, 5)
    assert (p.weight_concentration_prior, p.mean_precision_prior, p.degrees_of_freedom_prior, p.reg_covar, p.tol) == \
        (0.1, 0.1, 2.0, 1e-6, 1e-3) and tuple(p.mean_prior) == (0.0, 0.0)
    assert "ppk_bgmm_fit.hip" in open(os.path.join(ROOT, "poppunk_amd", "csrc", "Makefile")).read()
    assert _lib.sources_hash_now() == _lib.source_hash()


def test_argument_errors_are_status_codes_with_messages():
    lib = _lib.lib()
    for K in (0, 17, -1):
        with pytest.raises(ValueError, match=r"outside \[1, 16\]"):
            engine.bgmm_fit_params(K)
    for kw, msg in ((dict(max_iter=-1), "max_iter"), (dict(max_iter=5000), "max_iter"), (dict(n_init=0), "n_init"),
                    (dict(n_init=33), "n_init"), (dict(tol=-1.0), "priors"), (dict(degrees_of_freedom_prior=1.0), "degrees"),
                    (dict(weight_concentration_prior=0.0), "priors")):
        p = engine.bgmm_fit_params(2, **kw)
        st = _lib.BgmmState()
        z = np.zeros(14)
        f64p = C.POINTER(C.c_double)
        assert lib.ppk_bgmm_mstep(C.byref(p), z.ctypes.data_as(f64p), z.ctypes.data_as(f64p), z.ctypes.data_as(f64p),
                                  C.byref(st), None) == _lib.ERR_ARG
        assert msg in _lib.last_error()
    # a covariance that loses positive-definiteness: sums whose second moment is below the square of the first
    sums = np.array([[10.0, 5.0, 5.0, 1.0, 1.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match="component 0 lost positive-definiteness"):
        lib_mstep(1, sums, np.zeros((1, 2)), np.zeros((2, 2)), reg_covar=0.0)
    with pytest.raises(ValueError, match="not finite"):
        lib_mstep(1, np.array([[np.nan, 0, 0, 0, 0, 0, 0.0]]), np.zeros((1, 2)), np.eye(2))

    X = np.abs(np.random.default_rng(0).normal(0.3, 0.1, (50, 2))).astype(np.float32)
    lab = (np.arange(50) % 2).astype(np.int32)
    ok = engine.bgmm_fit_params(2)

    def fit(X=X, scale=(1.0, 1.0), params=ok, **kw):
        kw.setdefault("init_labels", lab[:X.shape[0]] if "index" not in kw else lab[:len(kw["index"])])
        with pytest.raises(ValueError) as e:
            engine.bgmm_fit(X, scale, params, **kw)
        return str(e.value)
    assert "fewer than 2 training rows (1)" in fit(X[:1])
    assert "fewer training rows (3) than components (4)" in fit(X[:3], params=engine.bgmm_fit_params(4), init_labels=lab[:3])
    bad = lab.copy()
    bad[7] = 2
    assert "label of training row 7 is outside [0, 2)" in fit(init_labels=bad)
    bad[7] = -1
    assert "label of training row 7" in fit(init_labels=bad)
    Xn = X.copy()
    Xn[31, 1], Xn[40, 0] = np.inf, np.nan
    assert "training row 31 is not finite" in fit(Xn)
    assert "training row 2 is not finite" in fit(Xn, index=np.array([3, 4, 40, 31]), init_labels=lab[:4])
    assert "scale must be positive" in fit(scale=(0.0, 1.0))
    assert "scale must be positive" in fit(scale=(1.0, -2.0))
    assert "index entry 1 is outside the matrix of 50 rows" in fit(index=np.array([0, 50, 2]), init_labels=lab[:3])
    assert "either the initial labels or the initial centres" in fit(init_labels=None)
    assert "either the initial labels or the initial centres" in fit(init_centres=np.zeros((5, 2, 2)))
    with pytest.raises(ValueError, match="one entry per training row"):
        engine.bgmm_fit(X, (1.0, 1.0), ok, init_labels=lab[:10])
    with pytest.raises(ValueError, match=r"\[n_init, K, 2\]"):
        engine.bgmm_fit(X, (1.0, 1.0), ok, init_centres=np.zeros((2, 2)))
    # device forms refuse before they touch a device
    s = np.array([1.0, 1.0], dtype=np.float32)
    sp = s.ctypes.data_as(C.POINTER(C.c_float))
    res, st = _lib.BgmmFitResult(), _lib.BgmmState()
    p = C.c_void_p(X.ctypes.data)
    assert lib.ppk_bgmm_fit_dev(p, 50, None, 0, sp, None, None, C.byref(ok), C.byref(res), None) == _lib.ERR_ARG
    assert lib.ppk_bgmm_fit_dev(None, 50, None, 0, sp, p, None, C.byref(ok), C.byref(res), None) == _lib.ERR_ARG
    assert lib.ppk_bgmm_stats_dev(p, 50, None, 0, sp, C.byref(st), p, None) == _lib.ERR_ARG and "K = 0" in _lib.last_error()
    assert lib.ppk_bgmm_kmeans_dev(p, 50, None, 0, sp, 17, np.zeros(34).ctypes.data_as(C.POINTER(C.c_double)), p, p, p,
                                   None) == _lib.ERR_ARG and "K = 17" in _lib.last_error()


def test_kmeanspp_draw_is_seeded_and_bounded():
    rng = np.random.default_rng(5)
    X = np.abs(rng.normal(0.4, 0.2, (10000, 2)))
    a = bgmm.initial_centres(lambda pos: X if pos is None else X[pos], 10000, (1.0, 1.0), 4, 42, 3)
    b = bgmm.initial_centres(lambda pos: X if pos is None else X[pos], 10000, (1.0, 1.0), 4, 42, 3)
    assert a.shape == (3, 4, 2) and np.array_equal(a, b) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a[1], bgmm.initial_centres(lambda pos: X[pos], 10000, (1.0, 1.0), 4, 43, 1)[0])
    seen = []
    bgmm.initial_centres(lambda pos: seen.append(pos) or X[pos], 10000, (1.0, 1.0), 2, 0, 1)
    assert seen[0].shape == (bgmm.SEED_SAMPLE,)
    # every centre is one of the (float32-scaled) rows; identical rows do not stall the draw
    rows = np.float32(X[:100])
    c = bgmm.initial_centres(lambda pos: rows, 100, (2.0, 2.0), 3, 1, 1)[0]
    scaled = (rows / np.float32(2.0)).astype(np.float64)
    assert all((scaled == ck).all(axis=1).any() for ck in c)
    same = np.full((10, 2), 0.25, dtype=np.float32)
    assert np.array_equal(bgmm.initial_centres(lambda pos: same, 10, (1.0, 1.0), 3, 1, 1)[0], np.full((3, 2), 0.25))


# ---- the exact reference and the inputs of the shape tests ---------------------------------------------------------------
def exact_close(got, want, scale, bar=1e-11):
    """(largest |got - want| / scale, whether it is within bar); where the scale is 0 the two must be equal."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if np.any(err[scale == 0] != 0) or not np.all(np.isfinite(err)):
        return np.inf, False
    d = float((err[scale > 0] / scale[scale > 0]).max()) if np.any(scale > 0) else 0.0
    return d, d <= bar


@pytest.mark.parametrize("case", cases())
def test_exact_sums_equal_the_plain_ones(case):
    g = case_of(golden(), case)
    K = int(g["K"])
    X = g["X"].astype(np.float64)
    S = ref_fit(X, g["labels0"], K, max_iter=1)["init"]
    lr = ref_log_resp(X, S)
    want, scale = ref_sums_exact(X, S, S["means"])
    assert np.all(scale[:, :1] > 0)
    d, ok = exact_close(ref_sums(X, np.exp(lr), lr, S["means"]), want, scale)
    assert ok, d
    _, xk, _ = ref_stats(X, one_hot(g["labels0"], K))
    want, scale = ref_sums_exact(X, g["labels0"], xk)
    d, ok = exact_close(ref_sums(X, one_hot(g["labels0"], K), None, xk), want, scale)
    assert ok, d
    assert np.array_equal(want[:, 0], np.bincount(g["labels0"], minlength=K)) and np.all(want[:, 6] == 0)
    assert np.array_equal(scale[:, 0], want[:, 0]) and np.array_equal(scale[:, 6], want[:, 0])


def test_counts_equal_explicit_repetition():
    _, xs, _, _, _ = shape_block()
    X = xs[:37]
    counts = np.array([(3 * i) % 5 for i in range(37)])             # zeros included
    rep = np.repeat(X, counts, axis=0)
    for K in (1, 5):
        S = shape_state(K)
        a, sa = ref_sums_exact(X, S, S["means"], counts)
        b, sb = ref_sums_exact(rep, S, S["means"])
        # (count * term rounds once where the repetition adds the term count times exactly: half an ulp per term)
        assert np.all(np.abs(a - b) <= 2 * EPS * sb) and np.all(np.abs(sa - sb) <= 4 * EPS * sb)
        lab = shape_labels(37, K)
        a, sa = ref_sums_exact(X, lab, S["means"], counts)
        b, sb = ref_sums_exact(rep, np.repeat(lab, counts), S["means"])
        assert np.all(np.abs(a - b) <= 2 * EPS * sb) and np.array_equal(a[:, 0], b[:, 0])
    for n in (1, 300, 4099, 4100, 524_289):
        assert np.array_equal(shape_counts(n), np.bincount(shape_rows(n), minlength=SHAPE_BLOCK))


def test_shape_inputs_meet_their_conditions():
    raw, xs, out, dup, src = shape_block()
    assert raw.dtype == np.float32 and raw.shape == (SHAPE_BLOCK, 2) and np.isfinite(raw).all() and np.isfinite(xs).all()
    assert tuple(SHAPE_SCALE) != (1.0, 1.0)
    assert out.size == SHAPE_OUTLIERS and dup.size == SHAPE_DUPLICATES
    assert np.array_equal(raw[dup], raw[src]) and not set(dup) & set(src) and not set(out) & (set(dup) | set(src))
    inl = np.setdiff1d(np.arange(SHAPE_BLOCK), out)
    assert xs[inl].min() > 0.0 and xs[inl].max() < 1.0
    assert np.hypot(*(xs[out] - 0.5).T).min() > 39.0
    for K in SHAPE_KS:
        S = shape_state(K)
        assert all(np.isfinite(S[k]).all() for k in ("a", "b", "beta", "means", "dof", "cov"))
        assert min(np.linalg.eigvalsh(c).min() for c in S["cov"]) > 0
        r = np.exp(ref_log_resp(xs, S))
        assert np.all(r.sum(axis=0) > 0)
        sums, scale = ref_sums_exact(xs[:300], S, S["means"])
        assert np.all(scale[:, 0] > 0) and np.isfinite(sums).all() and np.isfinite(scale).all()
    # the outliers: with two components every one of them leaves a single responsibility above 0
    r = np.exp(ref_log_resp(xs, shape_state(2)))
    assert np.all((r[out] == 0).sum(axis=1) == 1) and np.all(r[inl] > 0)
    assert sum(int((np.exp(ref_log_resp(xs, shape_state(K))) == 0).any()) for K in SHAPE_KS) >= 12


@pytest.mark.parametrize("n", [300, 4097])
def test_shape_centres_leave_no_label_to_a_rounding(n):
    X = shape_block()[1][:n]
    for K in SHAPE_KS:
        for centres in shape_centres(K, n):
            assert centres.shape == (K, 2) and np.isfinite(centres).all()
            d2 = np.sort(nearest_d2(X, centres), axis=1)
            if K > 1:
                assert np.all(d2[:, 1] - d2[:, 0] > 1e-9 * d2[:, 1])
                k = K // 2
                assert tuple(centres[k]) == PLANTED and not np.any(ref_nearest(X, centres) == k)
                assert nearest_d2(X, centres[k:k + 1]).min() > np.delete(nearest_d2(X, centres), k, axis=1).max()
        a, b = shape_centres(K, n)
        assert K <= 2 or np.any(ref_nearest(X, a) != ref_nearest(X, b))         # the second pass changes labels


def test_tied_set_is_exact_and_holds_every_tie():
    rows, nine, five = tied_set()
    X = rows.astype(np.float64)
    for a in (X, nine, five):
        assert np.array_equal(a * 64, np.round(a * 64)) and np.abs(a).max() < 4
    assert rows.shape[0] > 2048
    d2 = nearest_d2(X, nine[:5])
    ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    assert {2, 3, 4} <= set(ties.tolist())
    first = ref_nearest(X, nine[:5])
    across = (d2[:, 3] == d2.min(axis=1)) & (d2[:, 4] == d2.min(axis=1))
    assert np.any(across & (ties == 2)) and np.any(across & (ties == 3)) and np.all(first[across] <= 3)
    lab9 = ref_nearest(X, nine)
    assert not np.any(lab9 == 6) and all(np.any(lab9 == k) for k in (0, 1, 2, 3, 4, 5, 7, 8))
    lab5 = ref_nearest(X, five)
    assert set(lab5.tolist()) == {0, 1, 3}
