"""CPU tests of BGMM assignment: ppk_bgmm_prepare (no device), the model loader, and a numpy restatement of the
reference's assignment against tests/golden/bgmm_assign.npz and bgmm_assign_k.npz (tests/golden/make_golden_bgmm.py)."""
import os

import numpy as np
import pytest

from poppunk_amd import _lib
from poppunk_amd.models import BGMMModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")
GOLDEN_K = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign_k.npz")


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_k():
    """K = 1, 3, 5, 16 with odd row counts (make_golden_bgmm.py --k)"""
    return np.load(GOLDEN_K, allow_pickle=False)


def case_model(g, case):
    return BGMMModel(g[case + "_weights"], g[case + "_means"], g[case + "_covariances"], g[case + "_scale"],
                     g[case + "_within"].item(), g[case + "_between"].item())


def test_prepare_matches_scipy_cholesky():
    from scipy import linalg
    for g, case in [(g, case) for g in (golden(), golden_k()) for case in list(g["cases"])]:
        m = case_model(g, case).model
        for c, cv in enumerate(g[case + "_covariances"]):
            try:
                L = linalg.cholesky(cv, lower=True)
                assert m.jitter[c] == 0
            except linalg.LinAlgError:
                L = linalg.cholesky(cv + 1e-7 * np.eye(2), lower=True)
                assert m.jitter[c] == 1
            got = np.array([m.chol[c][0], m.chol[c][1], m.chol[c][2]])
            np.testing.assert_allclose(got, [L[0, 0], L[1, 0], L[1, 1]], rtol=1e-14, atol=0)
            const = np.log(g[case + "_weights"][c]) - 0.5 * (2 * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L))))
            np.testing.assert_allclose(m.log_const[c], const, rtol=1e-14)
            np.testing.assert_allclose([m.mean[c][0], m.mean[c][1]], g[case + "_means"][c], rtol=0)


def test_golden_covers_a_near_empty_component_and_both_scale_dtypes():
    g = golden()
    assert g["k4_weights"].min() < 0.01
    assert g["split_f32_scale"].dtype == np.float32 and g["split_f64_scale"].dtype == np.float64
    n = int(g["split_rows"])
    assert (g["split_f32_labels"][:n] != g["split_f64_labels"][:n]).all()
    assert case_model(g, "split_f32").model.scale_is_f64 == 0 and case_model(g, "split_f64").model.scale_is_f64 == 1


def test_lin_constants_restate_the_triangular_solve():
    g = golden()
    m = case_model(g, "k4").model
    xs = g["k4_X"][:50].astype(np.float64) / g["k4_scale"].astype(np.float64)
    for c in range(4):
        l = m.lin[c]
        z0 = xs[:, 0] * l[0] + l[1]
        z1 = xs[:, 1] * l[2] + (z0 * l[3] + l[4])
        d0, d1 = xs[:, 0] - m.mean[c][0], xs[:, 1] - m.mean[c][1]
        w0 = d0 / m.chol[c][0]
        w1 = (d1 - m.chol[c][1] * w0) / m.chol[c][2]
        np.testing.assert_allclose(z0, w0, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(z1, w1, rtol=1e-9, atol=1e-12)


def test_fallback_and_raise_where_the_reference_takes_them():
    g = golden()
    assert case_model(g, "jitter").model.n_jitter == 1
    assert case_model(g, "k2").model.n_jitter == 0
    with pytest.raises(ValueError, match="positive-definite"):
        case_model(g, "raise")


def test_prepare_rejects_bad_arguments():
    w, m, c = np.ones(1), np.zeros((1, 2)), np.eye(2)[None]
    with pytest.raises(ValueError, match="within_label"):
        BGMMModel(w, m, c, [1.0, 1.0], 1)
    K = _lib.BGMM_MAX_K + 1
    with pytest.raises(ValueError, match="K = 17"):
        BGMMModel(np.ones(K) / K, np.zeros((K, 2)), np.tile(np.eye(2), (K, 1, 1)), [1.0, 1.0], 0)
    assert BGMMModel(w, m, c, np.float32([1, 1]), 0).model.scale_is_f64 == 0
    assert BGMMModel(w, m, c, np.float64([1, 1]), 0).model.scale_is_f64 == 1


def test_from_npz_accepts_bgmm_and_refuses_other_fits(tmp_path):
    g = golden()
    p = tmp_path / "x_fit.npz"
    np.savez(p, weights=g["k2_weights"], means=g["k2_means"], covariances=g["k2_covariances"],
             within=g["k2_within"], between=g["k2_between"], scale=g["k2_scale"])
    m = BGMMModel.from_npz(str(p))
    assert m.within_label == g["k2_within"].item() and m.between_label == g["k2_between"].item()
    assert m.model.scale_is_f64 == 0 and m.n_components == 2
    with pytest.raises(ValueError, match="refine"):
        BGMMModel.from_npz({"intercept": np.zeros(2), "core_acc_intercepts": np.zeros(2), "scale": np.ones(2)})
    with pytest.raises(ValueError, match="DBSCAN"):
        BGMMModel.from_npz({"n_clusters": 3, "means": np.zeros((3, 2)), "maxs": np.zeros((3, 2)),
                            "mins": np.zeros((3, 2)), "scale": np.ones(2), "within": 0, "between": 1})
    with pytest.raises(ValueError, match="missing"):
        BGMMModel.from_npz({"weights": np.ones(1)})


def test_unfitted_model_raises():
    g = golden()
    m = case_model(g, "k2")
    m.fitted = False
    with pytest.raises(RuntimeError, match="unfitted"):
        m.assign(g["k2_X"])


def restated(X, weights, means, covariances, scale):
    """The reference's statement (bgmm.py:100-176, models.py:177-187) in numpy, for the golden's consistency."""
    from scipy import linalg
    from scipy.special import logsumexp
    xs = X / scale
    lpr = np.empty((X.shape[0], len(weights)))
    for c, (mu, cv) in enumerate(zip(means, covariances)):
        try:
            L = linalg.cholesky(cv, lower=True)
        except linalg.LinAlgError:
            L = linalg.cholesky(cv + 1e-7 * np.eye(2), lower=True)
        sol = linalg.solve_triangular(L, (xs - mu).T, lower=True).T
        lpr[:, c] = -0.5 * (np.sum(sol ** 2, axis=1) + 2 * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L))))
    lpr += np.log(weights)
    resp = np.exp(lpr - logsumexp(lpr, axis=1)[:, None])
    return resp.argmax(axis=1), resp.astype(X.dtype)


def test_numpy_restatement_matches_golden():
    for g, case in [(g, case) for g in (golden(), golden_k()) for case in list(g["cases"])]:
        X = g[case + "_X"]
        labels, resp = restated(X, g[case + "_weights"], g[case + "_means"], g[case + "_covariances"],
                                g[case + "_scale"])
        assert np.array_equal(labels, g[case + "_labels"]), case
        np.testing.assert_allclose(resp, g[case + "_resp"], rtol=1e-6, atol=1e-30)


def test_golden_k_has_no_undecided_row_and_every_component_matters():
    """What tests/test_gpu_bgmm_shapes.py relies on: every row of bgmm_assign_k.npz is decided by the rule of
    test_gpu_bgmm.py (so labels compare exactly on all of them), a kernel that skipped a component would mislabel a
    row (every component of k3 and k5, at least 12 of k16's 16, is some row's label), every row count is odd (the
    one-row tail of a kernel that takes two rows per lane), and the file is no larger than bgmm_assign.npz."""
    g = golden_k()
    assert list(g["cases"]) == ["k1", "k3", "k3_f64", "k5", "k16"]
    for case, K in (("k1", 1), ("k3", 3), ("k3_f64", 3), ("k5", 5), ("k16", 16)):
        gap, top, labels = g[case + "_gap"], g[case + "_top"], g[case + "_labels"]
        assert g[case + "_weights"].shape == (K,) and g[case + "_resp"].shape == (labels.shape[0], K)
        assert labels.shape[0] % 2 == 1, case
        assert (gap <= 1e-9 * np.maximum(1.0, np.abs(top))).sum() == 0, case
        assert np.unique(labels).size >= (12 if K == 16 else K), case
        assert 0 <= g[case + "_within"].item() < K
    assert (g["k1_labels"] == 0).all() and (g["k1_resp"] == 1.0).all()
    assert g["k5_within"].item() == 4 and g["k5_weights"].min() == 1e-4 and g["k16_weights"].min() == 1e-4
    assert g["k3_scale"].dtype == np.float32 and g["k3_f64_scale"].dtype == np.float64
    for case in ("k5", "k16"):      # correlated covariances, up to +-0.9
        cv = g[case + "_covariances"]
        rho = cv[:, 0, 1] / np.sqrt(cv[:, 0, 0] * cv[:, 1, 1])
        assert abs(rho.min() + 0.9) < 1e-12 and abs(rho.max() - 0.9) < 1e-12
    assert os.path.getsize(GOLDEN_K) <= os.path.getsize(GOLDEN)
