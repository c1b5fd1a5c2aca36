"""GPU tests of the density grids' second round: the wave pre-sum of the kde pass gives the sums'
bits at every group size, the first offender is the first in reading order whichever kind it is, the three models'
plot methods, plot_dbscan_results on both routes, more labels than one counts call takes, the sampled rows on the
raster route, and the values of contour_surfaces and distHistogram."""
import os

import numpy as np
import pytest

import density_model as dm
from poppunk_amd import engine, models, plot
from test_gpu_density import GRID, RecordingPlt, bgmm_of, dev, kde_dev, random_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return dm.load_golden()


# ---- the wave pre-sum: the same bits ------------------------------------------------------------------------------
@pytest.mark.parametrize("min_group", [1, 8, 64])
def test_kde_presum_gives_the_same_bits(ppk_option, golden, min_group):
    """1: every window found in the rounds is summed across the wave, single lanes included; 8: groups and lone lanes
    mix in one wave; 64: only a wave whose lanes all share a window."""
    ppk_option("density_kde_presum", min_group)
    x = golden["blobs3000_x"]
    scale = np.amax(x, axis=0)
    want, _ = dm.kde_sums(x, GRID, GRID, dm.H, scale, 40)
    got, _, _ = kde_dev(x, GRID, GRID, dm.H, scale)
    assert np.array_equal(got, want)
    # one row 100 000 times: every wave is one group (the last one ragged: 100 000 = 1562 * 64 + 32)
    row = np.array([[0.0123, 0.171]], dtype=np.float32)
    shift = engine.pair_sum_shift(100000)
    one, _ = dm.kde_sums(row, GRID, GRID, dm.H, scale, shift)
    got, _, _ = kde_dev(np.repeat(row, 100000, axis=0), GRID, GRID, dm.H, scale)
    assert np.array_equal(got, one * 100000)
    # rows crowded near the origin among spread ones, a ragged last chunk, a non-uniform non-square grid
    gx = np.array([0.0, 0.04, 0.1, 0.15, 0.22, 0.3, 0.37, 0.45, 0.5, 0.58, 0.66, 0.7, 0.81, 0.9, 0.95, 1.0])
    gy = np.linspace(0, 1, 12)
    x = random_rows(300007, 3)
    x[::3] *= np.float32(0.02)
    shift = engine.pair_sum_shift(len(x))
    want, _ = dm.kde_sums(x, gx, gy, 0.11, (1.5, 1.25), shift)
    got, _, _ = kde_dev(x, gx, gy, 0.11, (1.5, 1.25))
    assert np.array_equal(got, want)
    # an index list with repeats, and offenders among the lanes of a group
    idx = np.concatenate([np.full(70, 7), np.arange(2999, 2900, -1), np.full(70, 7)])
    want, _ = dm.kde_sums(golden["blobs3000_x"], GRID, GRID, dm.H, scale, 40, idx)
    got, _, rows = kde_dev(golden["blobs3000_x"], GRID, GRID, dm.H, scale, idx=idx, shift=40)
    assert rows == len(idx) and np.array_equal(got, want)
    idx[100] = 3000
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: index 100: row 3000 outside \[0, 3000\)"):
        kde_dev(golden["blobs3000_x"], GRID, GRID, dm.H, scale, idx=idx)


@pytest.mark.parametrize("min_group", [0, 8])
def test_kde_names_the_first_offender_of_either_kind(ppk_option, golden, min_group):
    ppk_option("density_kde_presum", min_group)
    x = golden["blobs3000_x"].copy()
    x[2100, 1] = np.nan
    scale = (1.0, 1.0)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: index 1: row 2100: value \(.*, nan\) is not finite"):
        kde_dev(x, GRID, GRID, dm.H, scale, idx=np.array([5, 2100, 9, 3000, 2100]))
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: index 1: row 3000 outside \[0, 3000\)"):
        kde_dev(x, GRID, GRID, dm.H, scale, idx=np.array([5, 3000, 9, 2100, -1]))


# ---- the models' plot methods -------------------------------------------------------------------------------------
def test_every_model_plots_and_needs_an_output_prefix(golden, tmp_path):
    pytest.importorskip("matplotlib")
    import torch
    x = golden["blobs500_x"]
    x_t = dev(x)
    out = str(tmp_path / "db")
    os.makedirs(out)
    bgmm = bgmm_of(x)
    y_t = bgmm.assign_dev(x_t)
    dbscan = models.DBSCANModel()
    y_db = dbscan.fit_dev(x_t, 100, 0.01)
    refine = models.RefineBoundary(scale=bgmm.scale, slope=2, optimal_x=0.4, optimal_y=0.5, core_boundary=0.3,
                                   accessory_boundary=0.45)
    for call in (lambda **kw: bgmm.plot(x_t, y_t, **kw), lambda **kw: dbscan.plot(x_t, **kw),
                 lambda **kw: refine.plot(x_t, **kw)):
        with pytest.raises(ValueError, match="plot needs outPrefix"):
            call()
        call(outPrefix=out)
    dbscan.plot(x, y_db.cpu().numpy(), outPrefix=out, raster_above=0)           # host arrays, the raster route
    refine.plot(x, refine.assign_dev(x_t).cpu().numpy(), outPrefix=out, raster_above=0)
    want = {"db_DPGMM_fit.png", "db_DPGMM_fit_contours.pdf", "db_dbscan.png", "db_refined_fit.png"}
    assert want <= set(os.listdir(out))
    assert all(os.path.getsize(os.path.join(out, f)) > 10000 for f in want)
    assert torch.equal(y_db, dbscan.assign_dev(x_t))


def recorded(monkeypatch):
    import matplotlib as mpl
    rec = RecordingPlt()
    rec.cm = mpl.cm
    monkeypatch.setattr(plot, "_pyplot", lambda: (mpl, rec))
    return mpl, rec


@pytest.mark.parametrize("n_clusters", [3, 40])
def test_plot_dbscan_results_on_both_routes(monkeypatch, tmp_path, n_clusters):
    """40 clusters and noise are 41 labels: more than one counts call takes (29 at the figure's size), so the raster
    route makes two passes."""
    pytest.importorskip("matplotlib.pyplot")
    mpl, rec = recorded(monkeypatch)
    x = random_rows(20000, 17)
    y = (np.arange(20000) % (n_clusters + 1)) - 1
    y[y == 2] = 1                                         # cluster 2 is empty: not drawn
    out = str(tmp_path / "fit")
    plot.plot_dbscan_results(dev(x), dev(y.astype(np.int32)), n_clusters, out)
    lines = [c for c in rec.calls if c[0] == "plot"]
    assert len(lines) == n_clusters and "imshow" not in rec.names()
    assert lines[0][2] == {"color": "k", "markersize": 1} and np.array_equal(lines[0][1][0], x[y == -1, 0])
    assert lines[1][2]["markersize"] == 2 and np.array_equal(lines[1][1][1], x[y == 0, 1])
    rec.calls.clear()
    plot.plot_dbscan_results(dev(x), dev(y.astype(np.int32)), n_clusters, out, raster_above=0)
    assert "plot" not in rec.names() and rec.names().count("imshow") == 1
    img = [c for c in rec.calls if c[0] == "imshow"][0][1][0]
    # the last label drawn wins a pixel: the highest cluster in it; noise only where there is nothing else
    (x0, inv_dx, nx, y0, inv_dy, ny), _ = plot.raster_for(np.amax(x, axis=0))
    ix = np.floor((x[:, 0].astype(np.float64) - x0) * inv_dx).astype(int)
    iy = np.floor((x[:, 1].astype(np.float64) - y0) * inv_dy).astype(int)
    top = np.full((ny, nx), -2)
    np.maximum.at(top, (iy, ix), y)
    colours = {k: np.asarray(c[2]["color"] if k >= 0 else mpl.colors.to_rgba("k"), dtype=np.float32)
               for k, c in zip(sorted(set(y.tolist())), lines)}
    assert img.shape == (ny, nx, 4) and np.all(img[top == -2] == 0)
    for k in sorted(colours):
        assert (top == k).any() and np.all(img[top == k] == mpl.colors.to_rgba(colours[k]))
    # the passes' counts on a small raster, bit for bit: 41 labels are two passes there, and 32 at most fit one
    raster = (-0.05, 40.0, 64, -0.05, 30.0, 48)
    want, outside = dm.counts(x, raster, y, -1, n_clusters + 1)
    for X, Y in ((dev(x), dev(y.astype(np.int32))), (x, y)):
        counts, got_out, _ = plot.label_rasters(X, Y, -1, n_clusters + 1, raster=raster)
        assert got_out == outside and counts.shape == want.shape and np.array_equal(counts, want)
    if n_clusters > 31:
        with pytest.raises(ValueError, match=r"labels outside \[-1, 39\)"):
            plot.label_rasters(dev(x), dev(y.astype(np.int32)), -1, n_clusters, raster=raster)
    assert [c[1][0] for c in rec.calls if c[0] == "savefig"] == [out + ".png"]


def test_plot_results_with_more_components_than_one_counts_call_takes(monkeypatch, tmp_path):
    pytest.importorskip("matplotlib.pyplot")
    mpl, rec = recorded(monkeypatch)
    K = 34
    x = random_rows(6000, 23)
    y = np.arange(6000) % K
    means = np.linspace(0.1, 0.9, K)[:, None] * np.ones((1, 2))
    covs = np.tile(np.eye(2) * 1e-3, (K, 1, 1))
    plot.plot_results(dev(x), dev(y.astype(np.int32)), means, covs, np.amax(x, axis=0), "BGMM", str(tmp_path / "fit"),
                      raster_above=0)
    img = [c for c in rec.calls if c[0] == "imshow"][0][1][0]
    (x0, inv_dx, nx, y0, inv_dy, ny), _ = plot.raster_for(np.amax(x, axis=0))
    ix = np.floor((x[:, 0].astype(np.float64) - x0) * inv_dx).astype(int)
    iy = np.floor((x[:, 1].astype(np.float64) - y0) * inv_dy).astype(int)
    top = np.full((ny, nx), -1)
    np.maximum.at(top, (iy, ix), y)
    for k in (0, 28, 29, K - 1):                  # (29 labels fit one pass at this size: both sides of the seam)
        colour = np.asarray(mpl.colors.to_rgba(plot.BGMM_COLOURS[k % 5]), dtype=np.float32)
        assert (top == k).any() and np.all(img[top == k] == colour)
    assert np.all(img[top == -1] == 0)


def test_plot_scatter_rasterises_the_rows_it_sampled(monkeypatch, tmp_path):
    """Above 1 000 000 rows kde_rows="sample" keeps 1 000 000: the raster route shows those rows, as the points route
    does, not the whole matrix."""
    pytest.importorskip("matplotlib.pyplot")
    mpl, rec = recorded(monkeypatch)
    n = 1000400
    x = random_rows(n, 31)
    x[:, 0] *= np.float32(0.5)
    x_t = dev(x)
    plot.plot_scatter(x_t, str(tmp_path), "Distances", kde_rows="sample", seed=77, raster_above=0)
    idx = plot.shuffle_indices(n, 77, 1000000)
    img = [c for c in rec.calls if c[0] == "imshow"][0][1][0]
    counts, outside, _ = plot.label_raster(x[idx])
    whole, _, _ = plot.label_raster(x, raster=plot.raster_for(np.amax(x[idx], axis=0))[0])
    assert outside == 0 and counts.sum() == 1000000
    assert np.array_equal(img[:, :, 3] > 0, counts[0] > 0)
    assert ((whole[0] > 0) != (counts[0] > 0)).any()          # (the whole matrix would light other pixels)
    rec.calls.clear()
    plot.plot_scatter(x_t, str(tmp_path), "Distances", kde_rows="sample", seed=77)
    sc = [c for c in rec.calls if c[0] == "scatter"][0]
    assert "imshow" not in rec.names() and len(sc[1][0]) == 1000000
    sx, sy = plot.scatter_points(x, np.amax(x[idx], axis=0), idx)
    assert np.array_equal(sc[1][0], sx) and np.array_equal(sc[1][1], sy)


# ---- plot_contours' surfaces and distHistogram, by value ----------------------------------------------------------
def test_contour_surfaces_by_value(golden):
    x = golden["blobs3000_x"]
    model = bgmm_of(x)
    y = model.assign_dev(dev(x))
    xx, yy, z, z_ll = plot.contour_surfaces(model, y)
    g = np.linspace(0, 1, 100)
    assert np.array_equal(xx, np.meshgrid(g, g)[0]) and z.shape == z_ll.shape == (100, 100)
    # z_ll[i, j] is the mixture's log density at core g[j], accessory g[i] -- the reference's transpose
    w, mu, cv = (np.asarray(a, dtype=np.float64) for a in (model.weights, model.means, model.covariances))
    for i, j in ((0, 0), (3, 80), (99, 10), (50, 50)):
        p = np.array([g[j], g[i]])
        dens = sum(w[c] * np.exp(-0.5 * (p - mu[c]) @ np.linalg.inv(cv[c]) @ (p - mu[c]))
                   / (2 * np.pi * np.sqrt(np.linalg.det(cv[c]))) for c in range(2))
        assert z_ll[i, j] == pytest.approx(np.log(dens), rel=1e-9, abs=1e-9)
    # z[i, j]: the within-strain minus the between-strain responsibility of the point (g[j], g[i]) as `assign` sees it,
    # divided by the model's scale (the reference passes the grid to BGMMFit.assign, which scales it).  The nodes
    # nearest the midpoint of the two means, where neither responsibility is saturated; the device's responsibilities
    # are float32 exponentials of Mahalanobis terms of order 10: 1e-4 is well above their rounding
    counts = np.bincount(y.cpu().numpy(), minlength=2)
    within, between = int(np.argmin(np.linalg.norm(mu, axis=1))), int(np.argmax(counts))
    mid = mu.mean(axis=0) * np.asarray(model.scale, dtype=np.float64)
    j0, i0 = int(np.argmin(np.abs(g - mid[0]))), int(np.argmin(np.abs(g - mid[1])))
    for i, j in ((i0, j0), (i0 + 1, j0), (i0, j0 + 1), (0, 0), (99, 99)):
        p = np.array([g[j], g[i]], dtype=np.float32) / np.asarray(model.scale, dtype=np.float32)
        lpr = np.array([np.log(w[c]) - 0.5 * (p - mu[c]) @ np.linalg.inv(cv[c]) @ (p - mu[c])
                        - 0.5 * np.log(np.linalg.det(cv[c])) for c in range(2)])
        resp = np.exp(lpr - lpr.max()) / np.exp(lpr - lpr.max()).sum()
        print("z[%d, %d] = %.6f, direct %.6f" % (i, j, z[i, j], resp[within] - resp[between]))
        assert z[i, j] == pytest.approx(resp[within] - resp[between], abs=1e-4)
    assert np.abs(z).max() <= 1.0 + 1e-6


def test_dist_histogram(monkeypatch, tmp_path):
    pytest.importorskip("matplotlib.pyplot")
    mpl, rec = recorded(monkeypatch)
    d = random_rows(500, 2)[:, 0]
    plot.distHistogram(dev(d), 3, str(tmp_path / "db"))
    h = [c for c in rec.calls if c[0] == "hist"][0]
    assert np.array_equal(h[1][0], d) and h[1][1] == 50 and h[2] == {"facecolor": "b", "alpha": 0.75}
    assert [c[1][0] for c in rec.calls if c[0] == "savefig"] == [str(tmp_path / "db") + "_rank_3_histogram.png"]
    assert ("title", ("Included nearest neighbour distances for rank 3",), {}) in rec.calls
