"""CPU tests of the density grids: the numpy restatement of the two rules (tests/density_model.py)
against what the reference's plot_scatter handed matplotlib (tests/golden/density.npz), the seeded sample's index list,
the raster helpers of poppunk_amd.plot, and the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import density_model as dm
from poppunk_amd import _lib, engine, plot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("blobs3000", "blobs500", "sample1500")
GRID = np.linspace(0, 1, 100)


@pytest.fixture(scope="module")
def golden():
    return dm.load_golden()


def case_rows(z, name):
    """(the matrix, the index list the reference's sample holds or None)."""
    x = z[name + "_x"]
    keep = int(z[name + "_max_plot_samples"])
    return x, (dm.shuffle_indices(len(x), int(z[name + "_seed"]), keep) if len(x) > keep else None)


def z_tolerance(cnt, shift, h, n, e_ref, z_rec):
    """Per cell: the fixed-point bound (half a unit of 2^-shift per row that reaches the cell, normalised) plus twice
    the reference side's own recorded rounding.  Nothing computed by the code under test enters it."""
    return cnt.T * 2.0 ** -(shift + 1) * dm.kde_norm(h, n) + 2.0 * e_ref * z_rec.max()


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_recorded_density(golden, name):
    x, idx = case_rows(golden, name)
    n = len(x) if idx is None else len(idx)
    scale = golden[name + "_scale"]
    assert np.array_equal(scale, np.amax(x if idx is None else x[idx], axis=0))
    shift = engine.pair_sum_shift(n)
    total, cnt = dm.kde_sums(x, GRID, GRID, dm.H, scale, shift, idx)
    z_rec = golden[name + "_z"]
    z = dm.z_from_sums(total, shift, dm.H, n)
    err = np.abs(z - z_rec)
    tol = z_tolerance(cnt, shift, dm.H, n, float(golden[name + "_e_ref"]), z_rec)
    print("%s: max |z - z_rec| = %.3g, smallest tolerance = %.3g" % (name, err.max(), tol.min()))
    assert np.all(err <= tol)
    assert float(golden[name + "_e_ref"]) < 1e-12
    # the contour's other arguments are the grid times the scale, and nine of ten levels
    xx, yy, _ = plot.get_grid(0, 1, 100)
    assert np.array_equal(golden[name + "_contour_x"], xx * scale[0])
    assert np.array_equal(golden[name + "_contour_y"], yy * scale[1])
    assert np.allclose(golden[name + "_levels"], np.linspace(z_rec.min(), z_rec.max(), 10)[1:], rtol=0, atol=0)


@pytest.mark.parametrize("name", CASES)
def test_scatter_arguments_and_the_seeded_index_list(golden, name):
    x, idx = case_rows(golden, name)
    if idx is not None:
        assert np.array_equal(idx, plot.shuffle_indices(len(x), int(golden[name + "_seed"]), len(idx)))
    before = x.copy()
    sx, sy = plot.scatter_points(x, golden[name + "_scale"], idx)
    assert sx.dtype == np.float32 and np.array_equal(sx, golden[name + "_scatter_x"])
    assert np.array_equal(sy, golden[name + "_scatter_y"])
    assert np.array_equal(x, before)            # the caller's matrix is not divided in place
    assert str(golden[name + "_savefig"]) == "out_dir_distanceDistribution.png"


def test_kde_restatement_edge_rules():
    # a row exactly on a node adds 2^shift there; a node exactly h away gets nothing (t == 0)
    gx = np.arange(5) / 64.0
    total, cnt = dm.kde_sums(np.array([[2 / 64.0, 1 / 64.0]], dtype=np.float32), gx, gx, 1 / 32.0, (1, 1), 20)
    assert total[2, 1] == 1 << 20 and total[0, 1] == 0 and total[4, 1] == 0 and total[2, 3] == 0
    assert total[1, 1] == (1 << 20) * 3 // 4 and cnt[0, 1] == 0 and cnt[1, 1] == 1
    # non-square grids keep [core node, accessory node]
    total, _ = dm.kde_sums(np.array([[0.0, 1.0]], dtype=np.float32), [0.0, 0.5], [0.0, 0.5, 1.0], 0.2, (1, 1), 10)
    assert total.shape == (2, 3) and total[0, 2] == 1 << 10 and total.sum() == 1 << 10


def test_counts_restatement_and_the_raster_helpers():
    raster, extent = plot.raster_for((0.5, 2.0), nx=10, ny=4, margin=0.0)
    assert extent == (0.0, 0.5, 0.0, 2.0) and raster == (0.0, 20.0, 10, 0.0, 2.0, 4)
    x = np.array([[0.0, 0.0], [0.5, 0.1], [0.49, 1.99], [-1e-9, 1.0], [0.26, 1.2]], dtype=np.float32)
    c, outside = dm.counts(x, raster, labels=[0, 1, 1, 0, -1], label_lo=-1, n_slots=3)
    assert outside == 2 and c.sum() == 3            # on the last edge and just below x0: outside
    assert c[1, 0, 0] == 1 and c[2, 3, 9] == 1 and c[0, 2, 5] == 1
    # where labels overlap, the later entry of the drawing order wins; empty pixels stay transparent
    counts = np.zeros((2, 1, 3), dtype=np.uint32)
    counts[0, 0, :2] = 1
    counts[1, 0, 1:] = 5
    img = plot.raster_image(counts, [(0, (1, 0, 0, 1)), (1, (0, 0, 1, 1))])
    assert img[0, 0].tolist() == [1, 0, 0, 1] and img[0, 1].tolist() == [0, 0, 1, 1] and img[0, 2].tolist() == [0, 0, 1, 1]
    assert plot.raster_image(counts, [(1, (0, 0, 1, 1)), (0, (1, 0, 0, 1))])[0, 1].tolist() == [1, 0, 0, 1]
    assert plot.raster_image(np.zeros((1, 2, 2), dtype=np.uint32), [(0, (1, 1, 1, 1))]).sum() == 0
    assert (plot.RASTER_NX, plot.RASTER_NY) == (1760, 1280)


def test_the_package_imports_without_matplotlib():
    import subprocess
    import sys
    code = ("import sys; sys.modules['matplotlib'] = None; sys.path.insert(0, %r); "
            "import poppunk_amd.plot as p; print(p.get_grid(0, 1, 2)[2].shape)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and "(4, 2)" in out.stdout, out.stderr


def test_new_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppk.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("ppk_density_kde_dev", "ppk_density_kde", "ppk_density_counts_dev", "ppk_density_counts"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.get_option("density_hot_table") in (0, 1)


def test_host_side_argument_errors_need_no_device():
    x = np.zeros((4, 2), dtype=np.float32)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: nx \* ny \+ nx \+ ny must be 1 \.\. 10240 .*100 x 100 fits"):
        engine.density_kde(x, np.linspace(0, 1, 110), GRID, 0.03, scale=(1, 1))
    with pytest.raises(RuntimeError, match="ppk_density_kde: gx is not strictly ascending at index 2"):
        engine.density_kde(x, [0.0, 0.5, 0.5], [0.0, 1.0], 0.03, scale=(1, 1))
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: gy\[1\] is not finite"):
        engine.density_kde(x, [0.0, 0.5], [0.0, np.inf], 0.03, scale=(1, 1))
    for h in (0.0, -1.0, np.nan, np.inf, 1e200):
        with pytest.raises(RuntimeError, match="ppk_density_kde: h = .* must be finite and positive"):
            engine.density_kde(x, [0.0, 0.5], [0.0, 1.0], h, scale=(1, 1))
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: scale\[1\] = 0 must be finite and positive"):
        engine.density_kde(x, [0.0, 0.5], [0.0, 1.0], 0.03, scale=(1, 0))
    with pytest.raises(RuntimeError, match="ppk_density_kde: shift must be 0 .. 40"):
        engine.density_kde(x, [0.0, 0.5], [0.0, 1.0], 0.03, scale=(1, 1), shift=41)
    with pytest.raises(RuntimeError, match="ppk_density_kde: no rows read"):
        engine.density_kde(x, [0.0, 0.5], [0.0, 1.0], 0.03, idx=np.zeros(0, dtype=np.int64))
    with pytest.raises(RuntimeError, match="ppk_density_counts: inv_dx and inv_dy must be finite and positive"):
        engine.density_counts(x, (0.0, 0.0, 4, 0.0, 1.0, 4))
    with pytest.raises(RuntimeError, match="ppk_density_counts: x0 and y0 must be finite"):
        engine.density_counts(x, (np.nan, 1.0, 4, 0.0, 1.0, 4))
    with pytest.raises(RuntimeError, match="ppk_density_counts: n_slots must be 1 without labels"):
        engine.density_counts(x, (0.0, 1.0, 4, 0.0, 1.0, 4), n_slots=2)
    with pytest.raises(RuntimeError, match=r"ppk_density_counts: n_slots \* nx \* ny must be at most 2\^26"):
        engine.density_counts(x, (0.0, 1.0, 4096, 0.0, 1.0, 4096), labels=np.zeros(4, dtype=np.int32), n_slots=8)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_without_a_device_the_entry_points_fail():
    x = np.zeros((4, 2), dtype=np.float32)
    with pytest.raises(RuntimeError):
        engine.density_kde(x, [0.0, 0.5], [0.0, 1.0], 0.03, scale=(1, 1))
    with pytest.raises(RuntimeError):
        engine.density_counts(x, (0.0, 1.0, 4, 0.0, 1.0, 4))


def test_the_library_checks_its_own_limits():
    """engine refuses these before it allocates; the library's own checks are reached through the bound symbol."""
    lib = _lib.lib()
    counts, outside = (C.c_uint32 * 4)(), C.c_longlong()
    for n_slots, nx, msg in ((0, 2, b"n_slots must be 1 .. 32"), (33, 2, b"n_slots must be 1 .. 32"),
                             (1, 0, b"nx and ny must be 1 .. 4096"), (1, 4097, b"nx and ny must be 1 .. 4096")):
        rc = lib.ppk_density_counts(None, 0, None, 0, n_slots, 0.0, 1.0, nx, 0.0, 1.0, 2, 0, counts, C.byref(outside))
        assert rc == _lib.ERR_ARG and lib.ppk_last_error() == b"ppk_density_counts: " + msg
    rc = lib.ppk_density_counts(None, 0, None, 0, 1, 0.0, 1.0, 2, 0.0, 1.0, 4097, 0, counts, C.byref(outside))
    assert rc == _lib.ERR_ARG and lib.ppk_last_error() == b"ppk_density_counts: nx and ny must be 1 .. 4096"
    assert _lib.get_option("density_kde_presum") in range(0, 65)


def test_log_likelihood_is_the_mixture_density():
    rng = np.random.RandomState(4)
    w = np.array([0.3, 0.7])
    mu = np.array([[0.1, 0.2], [0.6, 0.5]])
    cv = np.array([[[0.02, 0.005], [0.005, 0.01]], [[0.03, -0.01], [-0.01, 0.04]]])
    scale = np.array([2.0, 0.5])
    X = rng.uniform(0, 1, size=(50, 2)) * scale
    logprob, lpr = plot.log_likelihood(X, w, mu, cv, scale)
    Xs = X / scale
    want = np.stack([np.log(w[c]) - 0.5 * np.einsum("ni,ij,nj->n", Xs - mu[c], np.linalg.inv(cv[c]), Xs - mu[c])
                     - np.log(2 * np.pi) - 0.5 * np.log(np.linalg.det(cv[c])) for c in range(2)], axis=1)
    assert lpr.shape == (50, 2) and np.allclose(lpr, want, rtol=1e-10, atol=1e-10)
    assert np.allclose(logprob, np.log(np.exp(want).sum(axis=1)), rtol=1e-10, atol=1e-10)
    # a covariance without a Cholesky factor gets bgmm.py's 1e-7 on its diagonal
    flat = np.array([[[1.0, 1.0], [1.0, 1.0]]])
    lp, _ = plot.log_likelihood(np.array([[0.5, 0.5]]), [1.0], [[0.5, 0.5]], flat, [1.0, 1.0])
    assert np.isfinite(lp).all()
