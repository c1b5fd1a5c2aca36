"""GPU tests of the BGMM fit's passes at every component count, row count and grid shape its kernels branch on
(bgmm_stats_kernel<MODE_EM | MODE_LABEL | MODE_NEAREST> and bgmm_final_kernel), against
tests/test_bgmm_fit_host.py's ref_sums_exact: float64 terms summed with math.fsum, so the reference has no summation
error of its own, and a scale per sum that carries the error a term can have.  Bar: 1e-11 of that scale.

The inputs come from one generator (H.shape_block, H.shape_state, H.shape_centres, H.tied_set), whose conditions --
finite rows, positive-definite states, S r > 0 for every component, no label that hangs on a rounding, exact ties --
tests/test_bgmm_fit_host.py asserts on the CPU.  A row count above the block's 4 099 repeats the block cyclically and
the reference takes the same rows through `counts`.

What each test reaches (the grid is ceil(n / 2048) workgroups of 256, at most 1 024; components go four to a sweep):
  test_em_pass_every_k           MODE_EM, 1 to 4 sweeps and every tail of the last, grid 3 and grid 1 with a 44-row wave
  test_em_pass_row_counts        MODE_EM at one lane, one wave, one workgroup, grid 1 -> 2 -> 3; nothing written around
                                 the output; rows that start one row into an allocation
  test_em_pass_grid_shapes       MODE_EM at grid 256 -> 257 (bgmm_final_kernel's strided term), at the cap (a ninth row
                                 for some threads) and at sixteen rows a thread
  test_index_entries_outside_the_matrix_add_nothing   the index test before the dereference, MODE_EM and MODE_NEAREST
  test_nearest_pass_every_k_and_designed_ties         MODE_NEAREST: labels, changed, the (d2, index) rule, later sweeps
  test_label_pass_through_the_fit                     MODE_LABEL (ppk_bgmm_fit_dev, max_iter = 0), the prior's two passes
  test_two_iterations_at_grid_shapes                  the three modes chained by the fit at grid 2 and 257
Each prints its worst |got - want| / scale (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_bgmm_fit_host as H  # noqa: E402
from test_gpu_bgmm_fit import bits, close, cuda, embed, same_bits  # noqa: E402

from poppunk_amd import _lib, engine  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-11
ONE = (1.0, 1.0)
PAD = 64                                    # sentinel elements before and after an output
SENTINEL = 0x7ff80000deadbeef               # (a NaN's bits: compared as integers)
LAB_SENTINEL = -7
INT64_MIN = -2 ** 63


@functools.lru_cache(maxsize=None)
def block_dev():
    """The block on the device: (its rows, a larger matrix that holds them among NaN and other rows, their places)."""
    raw = H.shape_block()[0]
    big, idx = embed(raw, 3)
    return cuda(raw.copy()), cuda(big), cuda(idx)          # (a copy: the generator's arrays are read-only)


def rows_dev(n):
    """n rows, contiguous: the block repeated cyclically."""
    raw_t = block_dev()[0]
    return raw_t[:n] if n <= H.SHAPE_BLOCK else raw_t[torch.arange(n, device="cuda") % H.SHAPE_BLOCK]


def index_dev(n):
    """The same n rows as places in block_dev()'s larger matrix."""
    idx_t = block_dev()[2]
    return idx_t[:n] if n <= H.SHAPE_BLOCK else idx_t[torch.arange(n, device="cuda") % H.SHAPE_BLOCK]


def rows_host(n):
    """(the n scaled rows in float64, the raw float32 rows)"""
    raw, xs = H.shape_block()[:2]
    return xs[H.shape_rows(n)], raw[H.shape_rows(n)]


def meets(got, want_and_scale, what, worst):
    want, scale = want_and_scale
    d, ok = H.exact_close(got, want, scale, BAR)
    assert ok, (what, d)
    worst.append(d)


def exact_em(K, n):
    """The reference of an E-step pass over n rows: the block's terms, each times how often its row occurs."""
    S = H.shape_state(K)
    xs = H.shape_block()[1]
    if n <= H.SHAPE_BLOCK:
        return H.ref_sums_exact(xs[:n], S, S["means"])
    return H.ref_sums_exact(xs, S, S["means"], H.shape_counts(n))


# ---- 1. the E-step pass at every K --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", H.SHAPE_KS)
def test_em_pass_every_k(K):
    st = H.state_from_ref(H.shape_state(K), K)
    big_t = block_dev()[1]
    worst = []
    for n in (4097, 300):                   # grid 3, every thread at least two rows; grid 1, the last wave has 44 rows
        got_c = engine.bgmm_stats_dev(rows_dev(n), st, H.SHAPE_SCALE).cpu().numpy()
        got_i = engine.bgmm_stats_dev(big_t, st, H.SHAPE_SCALE, index_t=index_dev(n)).cpu().numpy()
        assert np.array_equal(bits(got_c), bits(got_i)), n
        meets(got_c, exact_em(K, n), (K, n), worst)
    print("em pass K=%d: max |d| / scale = %.2e" % (K, max(worst)))


# ---- 2. the E-step pass at every row count up to three workgroups -------------------------------------------------------
def stats_between_sentinels(rows_ptr, n_rows, idx_t, st):
    """ppk_bgmm_stats_dev into the middle of a sentinel-filled buffer: the [K, 7] sums, after checking every sentinel."""
    K = st.K
    buf = torch.full((2 * PAD + K * 7,), SENTINEL, dtype=torch.int64, device="cuda")
    _, sp = engine._fit_scale(H.SHAPE_SCALE)
    ip, ni = (None, 0) if idx_t is None else (C.c_void_p(idx_t.data_ptr()), idx_t.shape[0])
    rc = _lib.lib().ppk_bgmm_stats_dev(C.c_void_p(rows_ptr), n_rows, ip, ni, sp, C.byref(st),
                                       C.c_void_p(buf.data_ptr() + 8 * PAD), engine._stream_ptr(0))
    _lib.check(rc, "ppk_bgmm_stats_dev")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:PAD] == SENTINEL).all() and (h[PAD + K * 7:] == SENTINEL).all(), "sums written outside [K, 7]"
    return h[PAD:PAD + K * 7].view(np.float64).reshape(K, 7)


@pytest.mark.parametrize("K", (2, 5, 16))
def test_em_pass_row_counts(K):
    """One sweep, one sweep and a tail of one, four sweeps; a lane, a wave, a workgroup and the grid going 1 -> 2 -> 3.
    Below K rows some components receive next to nothing: the scale is then as small and the case stays."""
    st = H.state_from_ref(H.shape_state(K), K)
    raw_t, big_t, _ = block_dev()
    worst = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097):
        want = exact_em(K, n)
        # the rows start one row into a larger allocation whose other rows are NaN
        buf = torch.full((n + 2, 2), float("nan"), dtype=torch.float32, device="cuda")
        buf[1:1 + n] = raw_t[:n]
        got_o = stats_between_sentinels(buf.data_ptr() + 8, n, None, st)
        meets(got_o, want, (K, n, "offset"), worst)
        got_i = stats_between_sentinels(big_t.data_ptr(), big_t.shape[0], index_dev(n), st)
        assert np.array_equal(bits(got_o), bits(got_i)), (K, n)
    print("em row counts K=%d: max |d| / scale = %.2e" % (K, max(worst)))


# ---- 3. the E-step pass at the grid's thresholds ------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 5, 16))
def test_em_pass_grid_shapes(K):
    st = H.state_from_ref(H.shape_state(K), K)
    big_t = block_dev()[1]
    worst = []
    sizes = (524_288, 524_289,              # grid 256 -> 257: the first strided term of bgmm_final_kernel
             2_097_152, 2_097_153,          # the cap of 1 024 workgroups: some threads take a ninth row
             2 * 2_097_152 + 5)             # every thread takes at least sixteen rows
    for n in sizes:
        got = engine.bgmm_stats_dev(rows_dev(n), st, H.SHAPE_SCALE).cpu().numpy()
        meets(got, exact_em(K, n), (K, n), worst)
        if n == sizes[-1]:
            got_i = engine.bgmm_stats_dev(big_t, st, H.SHAPE_SCALE, index_t=index_dev(n)).cpu().numpy()
            assert np.array_equal(bits(got), bits(got_i)), (K, n)
    print("em grid shapes K=%d: max |d| / scale = %.2e" % (K, max(worst)))


# ---- 4. index entries outside the matrix --------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 5, 16))
def test_index_entries_outside_the_matrix_add_nothing(K):
    """include/ppk.h calls such an entry a precondition violation that contributes nothing.  Nothing here reads out of
    bounds: the kernel tests the index before it dereferences, and that test is what is pinned."""
    S = H.shape_state(K)
    st = H.state_from_ref(S, K)
    _, big_t, idx_t = block_dev()
    n_rows = big_t.shape[0]
    xs = H.shape_block()[1]
    bad = np.array([-1, n_rows, n_rows + 7, INT64_MIN], dtype=np.int64)
    worst = []
    for n in (300, 4097):
        valid = idx_t[:n].cpu().numpy()
        index = np.concatenate([bad, valid[:n // 2], bad, valid[n // 2:], bad])
        is_valid = (index >= 0) & (index < n_rows)
        assert int(is_valid.sum()) == n and not is_valid[0] and not is_valid[-1] and not is_valid[4 + n // 2]
        index_t = cuda(index)
        got = engine.bgmm_stats_dev(big_t, st, H.SHAPE_SCALE, index_t=index_t).cpu().numpy()
        meets(got, H.ref_sums_exact(xs[:n], S, S["means"]), (K, n, "em"), worst)
        # the k-means pass: the labels at the invalid places keep what they held, and are not counted as changed
        centres = H.shape_centres(K, n)[0]
        want = H.ref_nearest(xs[:n], centres)
        lab_t = torch.full((index.shape[0],), LAB_SENTINEL, dtype=torch.int32, device="cuda")
        for changed_want in (n, 0):
            sums_t, changed_t = engine.bgmm_kmeans_dev(big_t, centres, H.SHAPE_SCALE, lab_t, index_t=index_t)
            labels = lab_t.cpu().numpy()
            assert np.array_equal(labels[is_valid], want) and (labels[~is_valid] == LAB_SENTINEL).all(), (K, n)
            assert int(changed_t.item()) == changed_want, (K, n)
            sums = sums_t.cpu().numpy()
            assert np.array_equal(sums[:, 0], np.bincount(want, minlength=K).astype(np.float64))
            meets(sums, H.ref_sums_exact(xs[:n], want, centres), (K, n, "nearest"), worst)
    print("outside entries K=%d: max |d| / scale = %.2e" % (K, max(worst)))


# ---- 5. the nearest-centre pass -----------------------------------------------------------------------------------------
def tied_pass(centres):
    """One pass over the tied set from labels of -1: everything is exact in double, so everything is compared exactly."""
    rows = H.tied_set()[0]
    X = rows.astype(np.float64)
    K, n = centres.shape[0], rows.shape[0]
    lab_t = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sums_t, changed_t = engine.bgmm_kmeans_dev(cuda(rows.copy()), centres, ONE, lab_t)
    want = H.ref_nearest(X, centres)                                        # (np.argmin: the lower index on ties)
    assert np.array_equal(lab_t.cpu().numpy(), want), K
    assert int(changed_t.item()) == n
    assert np.array_equal(sums_t.cpu().numpy(), H.ref_sums(X, H.one_hot(want, K), None, centres)), K
    return sums_t.cpu().numpy(), want


@pytest.mark.parametrize("K", H.SHAPE_KS)
def test_nearest_pass_every_k_and_designed_ties(K):
    xs = H.shape_block()[1]
    worst = []
    for n in (300, 4097):
        X = xs[:n]
        first, second = H.shape_centres(K, n)
        lab_t = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        labels = np.full(n, -1, dtype=np.int32)
        for centres in (first, second):                                     # from -1, then from the first pass's labels
            sums_t, changed_t = engine.bgmm_kmeans_dev(rows_dev(n), centres, H.SHAPE_SCALE, lab_t)
            want = H.ref_nearest(X, centres)
            assert np.array_equal(lab_t.cpu().numpy(), want), (K, n)
            assert int(changed_t.item()) == int((want != labels).sum()), (K, n)
            labels = want
            sums = sums_t.cpu().numpy()
            assert np.array_equal(sums[:, 0], np.bincount(want, minlength=K).astype(np.float64)), (K, n)
            if K > 1:
                assert np.all(sums[K // 2] == 0), (K, n)                     # the planted centre: nothing at all
            meets(sums, H.ref_sums_exact(X, want, centres), (K, n), worst)
    print("nearest pass K=%d: max |d| / scale = %.2e" % (K, max(worst)))
    _, nine, five = H.tied_set()
    if K == 5:
        # ties of two, three and four centres, one across the edge between components 3 and 4; then identical centres
        tied_pass(nine[:5])
        sums, want = tied_pass(five)
        assert np.all(sums[[2, 4]] == 0) and set(want.tolist()) == {0, 1, 3}
    if K == 9:
        # the later sweeps read the label the first sweep wrote (it was -1 before): components 4 to 8
        sums, want = tied_pass(nine)
        assert np.all(sums[6] == 0) and np.all(sums[[4, 5, 7, 8], 0] > 0)
        assert np.array_equal(sums[4:, 0], np.bincount(want, minlength=9)[4:].astype(np.float64))


# ---- 6. the label pass, through the fit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 3, 5, 16))
def test_label_pass_through_the_fit(K):
    """MODE_LABEL is reachable only through the fit: max_iter = 0 stops after the initialisation.  Bars: cov_prior and
    train_mean 1e-12 of sqrt(var var) and sqrt(var) (centred sums of n terms, as the fixture's init comparison has it);
    the parameters 1e-10 max(1, |value|), the whole-matrix test's (no recorded order spread at these sizes)."""
    p = engine.bgmm_fit_params(K, n_init=1, max_iter=0)
    sizes = (K + 1, 257, 2049, 524_289)
    worst_prior, worst_par = 0.0, 0.0
    for n in sizes:
        X, raw = rows_host(n)
        labels = H.shape_labels(n, K)
        res = engine.bgmm_fit_dev(rows_dev(n), H.SHAPE_SCALE, p, init_labels_t=cuda(labels))
        assert res.n_iter == 0 and not res.converged and res.n_train == n
        W0 = np.cov(X.T).reshape(2, 2)
        sd = np.sqrt(np.diag(W0))
        d_cov, ok_cov = close(res.cov_prior, W0, 1e-12, scale=np.outer(sd, sd))
        d_mean, ok_mean = close(res.train_mean, X.mean(axis=0), 1e-12, scale=sd)
        assert ok_cov and ok_mean, (K, n, d_cov, d_mean)
        want = H.ref_params(H.ref_fit(X, labels, K, max_iter=1)["init"])
        d_par = max(close(getattr(res, k), want[k], scale=np.maximum(1.0, np.abs(want[k])))[0] for k in H.PARAM_KEYS)
        assert d_par <= 1e-10, (K, n, d_par)
        worst_prior, worst_par = max(worst_prior, d_cov, d_mean), max(worst_par, d_par)
        if n == sizes[-1]:
            host = engine.bgmm_fit(raw, H.SHAPE_SCALE, p, init_labels=labels)
            assert same_bits(res, host) and np.array_equal(bits(res.cov_prior), bits(host.cov_prior))
    print("label pass K=%d: prior %.2e of sqrt(var var), parameters %.2e of max(1, |value|)" % (K, worst_prior, worst_par))


# ---- 7. two iterations of the fit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2049, 524_289))
def test_two_iterations_at_grid_shapes(n):
    """K = 5 from the labels of one k-means pass, against the restatement on float64 rows at the whole-matrix test's
    bars: parameters 1e-10 max(1, |value|), the bound 1e-11 of itself."""
    K = 5
    X, _ = rows_host(n)
    centres = np.delete(H.shape_centres(K + 1, 4097)[0], (K + 1) // 2, axis=0)          # (without the planted centre)
    lab_t = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    engine.bgmm_kmeans_dev(rows_dev(n), centres, H.SHAPE_SCALE, lab_t)
    labels = lab_t.cpu().numpy()
    assert np.array_equal(labels, H.ref_nearest(X, centres))
    p = engine.bgmm_fit_params(K, n_init=1, max_iter=2)
    got = engine.bgmm_fit_dev(rows_dev(n), H.SHAPE_SCALE, p, init_labels_t=lab_t)
    again = engine.bgmm_fit_dev(rows_dev(n), H.SHAPE_SCALE, p, init_labels_t=lab_t)
    assert same_bits(got, again)
    want = H.ref_fit(X, labels, K, max_iter=2)
    assert got.n_iter == 2 == want["n_iter"]
    d_par = max(close(getattr(got, k), want[k], scale=np.maximum(1.0, np.abs(want[k])))[0] for k in H.PARAM_KEYS)
    d_lb = float((np.abs(got.lower_bounds - want["lower_bounds"]) / np.abs(want["lower_bounds"])).max())
    print("two iterations n=%d: parameters %.2e of max(1, |value|), bound (relative) %.2e" % (n, d_par, d_lb))
    assert d_par <= 1e-10 and d_lb <= 1e-11
