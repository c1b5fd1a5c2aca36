"""GPU tests of the density grids (ppk_density_kde*, ppk_density_counts*, poppunk_amd.plot): the sums
and counts bit for bit against the numpy restatement of the two rules (tests/density_model.py), the density against what
the reference's plot_scatter handed matplotlib (tests/golden/density.npz), every argument error by its message, and
the plots' files and routes."""
import os

import numpy as np
import pytest

import density_model as dm
from poppunk_amd import engine, plot

pytestmark = pytest.mark.gpu

GRID = np.linspace(0, 1, 100)
CASES = ("blobs3000", "blobs500", "sample1500")


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


@pytest.fixture(scope="module")
def golden():
    return dm.load_golden()


@pytest.fixture(scope="module")
def blobs(golden):
    """The 3 000-row matrix, its column maxima and its sums on the reference's grid at the default shift."""
    x = golden["blobs3000_x"]
    scale = np.amax(x, axis=0)
    shift = engine.pair_sum_shift(len(x))
    total, cnt = dm.kde_sums(x, GRID, GRID, dm.H, scale, shift)
    return x, scale, shift, total, cnt


def kde_dev(x, gx, gy, h, scale, idx=None, shift=None):
    s, used_shift, rows = engine.density_kde_dev(dev(x), gx, gy, h, scale=scale, idx_t=None if idx is None else dev(idx),
                                                 shift=shift)
    return s.cpu().numpy(), used_shift, rows


def random_rows(n, seed):
    rng = np.random.RandomState(seed)
    return np.abs(rng.normal(0.3, 0.25, size=(n, 2))).astype(np.float32)


# ---- the Epanechnikov sums, bit for bit ---------------------------------------------------------------------------
def test_kde_reference_grid_equals_restatement(blobs):
    x, scale, shift, total, _ = blobs
    got, used_shift, rows = kde_dev(x, GRID, GRID, dm.H, scale)
    assert used_shift == shift == 40 and rows == 3000
    assert got.dtype == np.int64 and got.shape == (100, 100) and np.array_equal(got, total)
    # the column maxima taken on the device are np.amax's, and divide to the same sums
    s, _, _, used = engine.density_kde_dev(dev(x), GRID, GRID, dm.H, return_scale=True)
    assert used.dtype == np.float32 and np.array_equal(used, scale) and np.array_equal(s.cpu().numpy(), total)
    # the host-array twin
    s, _, rows, used = engine.density_kde(x, GRID, GRID, dm.H)
    assert rows == 3000 and np.array_equal(used, scale) and np.array_equal(s, total)


def test_kde_wide_bandwidth_on_a_non_square_non_uniform_grid(golden):
    x = golden["blobs500_x"]
    gx = np.array([-0.3, 0.0, 0.07, 0.2, 0.55, 0.9, 1.4])
    gy = np.array([-0.1, 0.25, 0.3, 0.8, 1.2])
    scale = np.amax(x, axis=0)
    want, cnt = dm.kde_sums(x, gx, gy, 2.0, scale, 40)
    assert cnt.min() == 500                      # every cell sees every row
    got, _, _ = kde_dev(x, gx, gy, 2.0, scale, shift=40)
    assert got.shape == (7, 5) and np.array_equal(got, want)


def test_kde_bandwidth_narrower_than_the_spacing(blobs):
    x, scale, shift, _, _ = blobs
    want, cnt = dm.kde_sums(x, GRID, GRID, 0.004, scale, shift)
    assert 0 < cnt.sum() < len(x)                # most rows hit one cell or none
    got, _, _ = kde_dev(x, GRID, GRID, 0.004, scale)
    assert np.array_equal(got, want)


def test_kde_rows_on_nodes_and_exactly_h_from_nodes():
    g = np.arange(65) / 64.0
    rng = np.random.RandomState(5)
    x = (rng.randint(0, 65, size=(400, 2)) / 64.0).astype(np.float32)
    want, cnt = dm.kde_sums(x, g, g, 1 / 32.0, (1, 1), 30)
    # a row on node (a, b) reaches that node and its eight neighbours one step away; the nodes two steps away are at
    # distance exactly h: t == 0 there, and nothing is added
    assert cnt.sum() == sum((min(a, 1) + 1 + min(64 - a, 1)) * (min(b, 1) + 1 + min(64 - b, 1))
                            for a, b in (x * 64).astype(int))
    got, _, _ = kde_dev(x, g, g, 1 / 32.0, (1, 1), shift=30)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n_rows", [0, 1, 300007])
def test_kde_row_counts(n_rows):
    """300 007 rows: 74 workgroups of one 4 096-row chunk each, a ragged last one, and the cross-workgroup flush."""
    gx = np.array([0.0, 0.04, 0.1, 0.15, 0.22, 0.3, 0.37, 0.45, 0.5, 0.58, 0.66, 0.7, 0.81, 0.9, 0.95, 1.0])
    gy = np.linspace(0, 1, 12)
    x = random_rows(n_rows, 3)
    shift = engine.pair_sum_shift(n_rows)
    want, _ = dm.kde_sums(x, gx, gy, 0.11, (1.5, 1.25), shift)
    got, used_shift, rows = kde_dev(x, gx, gy, 0.11, (1.5, 1.25))
    assert used_shift == shift and rows == n_rows and np.array_equal(got, want)
    if n_rows == 0:
        assert not want.any()
    if n_rows > 1:
        assert want.sum() > 0


def test_kde_several_chunks_per_workgroup():
    """2 200 003 rows are 538 chunks of 4 096: more than the two workgroups per CU the launch starts on 256 CUs, so
    workgroups take a second chunk.  A 4 x 3 grid keeps the dense restatement quick."""
    x = random_rows(2200003, 8)
    gx, gy = np.array([0.0, 0.2, 0.5, 0.9]), np.array([0.1, 0.4, 0.8])
    shift = engine.pair_sum_shift(len(x))
    assert shift == 62 - 22
    want, _ = dm.kde_sums(x, gx, gy, 0.35, (1, 1), shift)
    got, _, _ = kde_dev(x, gx, gy, 0.35, (1, 1))
    assert np.array_equal(got, want)


def test_kde_maximum_contention(blobs):
    _, scale, _, _, _ = blobs
    row = np.array([[0.0123, 0.171]], dtype=np.float32)
    shift = engine.pair_sum_shift(100000)
    one, cnt = dm.kde_sums(row, GRID, GRID, dm.H, scale, shift)
    assert cnt.sum() > 20
    got, _, _ = kde_dev(np.repeat(row, 100000, axis=0), GRID, GRID, dm.H, scale)
    assert np.array_equal(got, one * 100000)


def test_kde_index_lists(blobs):
    x, scale, _, _, _ = blobs
    idx = np.concatenate([np.arange(2999, 1500, -1), [7, 7, 7, 0, 2999], np.arange(100, 160), np.arange(130, 90, -1)])
    shift = engine.pair_sum_shift(len(idx))
    want, _ = dm.kde_sums(x, GRID, GRID, dm.H, scale, shift, idx)
    got, _, rows = kde_dev(x, GRID, GRID, dm.H, scale, idx=idx)
    assert rows == len(idx) and np.array_equal(got, want)
    # the scale taken from the rows read only
    sub = np.arange(0, 3000, 7)
    s, _, _, used = engine.density_kde_dev(dev(x), GRID, GRID, dm.H, idx_t=dev(sub), return_scale=True)
    assert np.array_equal(used, np.amax(x[sub], axis=0))
    assert np.array_equal(s.cpu().numpy(), dm.kde_sums(x, GRID, GRID, dm.H, used, 40, sub)[0])
    s, _, rows, _ = engine.density_kde(x, GRID, GRID, dm.H, scale=scale, idx=idx)
    assert rows == len(idx) and np.array_equal(s, want)
    # an empty list reads nothing
    got, _, rows = kde_dev(x, GRID, GRID, dm.H, scale, idx=np.zeros(0, dtype=np.int64))
    assert rows == 0 and not got.any()


def test_kde_same_bits_on_every_call_and_for_any_row_order(blobs):
    x, scale, _, total, _ = blobs
    a, _, _ = kde_dev(x, GRID, GRID, dm.H, scale)
    b, _, _ = kde_dev(x, GRID, GRID, dm.H, scale)
    c, _, _ = kde_dev(x[np.random.RandomState(1).permutation(len(x))], GRID, GRID, dm.H, scale)
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, total)


# ---- the density against the reference's recorded contour arguments -----------------------------------------------
@pytest.mark.parametrize("as_tensor", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_scatter_density_equals_the_recorded_plot_arguments(golden, name, as_tensor):
    """|z_dev - z_rec| <= cnt_g * 2^-(shift + 1) * norm + 2 * e_ref * max z_rec per cell: the fixed-point bound from the
    rows that reach the cell (counted on the host) plus twice the reference side's own recorded rounding."""
    x = golden[name + "_x"]
    keep = int(golden[name + "_max_plot_samples"])
    before = x.copy()
    sd = plot.scatter_density(dev(x) if as_tensor else x, kde_rows="sample", max_plot_samples=keep,
                              seed=int(golden[name + "_seed"]))
    assert np.array_equal(x, before)
    n = min(len(x), keep)
    assert sd.rows_read == n and (sd.idx is None) == (len(x) <= keep)
    assert np.array_equal(sd.scale, golden[name + "_scale"])
    _, cnt = dm.kde_sums(x, GRID, GRID, dm.H, sd.scale, sd.shift, sd.idx)
    z_rec = golden[name + "_z"]
    tol = cnt.T * 2.0 ** -(sd.shift + 1) * dm.kde_norm(dm.H, n) + 2.0 * float(golden[name + "_e_ref"]) * z_rec.max()
    err = np.abs(sd.z - z_rec)
    print("%s: max |z_dev - z_rec| = %.3g, smallest tolerance %.3g" % (name, err.max(), tol.min()))
    assert sd.z.shape == (100, 100) and np.all(err <= tol)
    assert np.array_equal(sd.xx * sd.scale[0], golden[name + "_contour_x"])
    assert np.array_equal(sd.yy * sd.scale[1], golden[name + "_contour_y"])
    assert np.allclose(sd.levels[1:], golden[name + "_levels"], rtol=0, atol=2 * tol.max())
    sx, sy = plot.scatter_points(dev(x) if as_tensor else x, sd.scale, sd.idx)
    assert np.array_equal(sx, golden[name + "_scatter_x"]) and np.array_equal(sy, golden[name + "_scatter_y"])


def test_scatter_density_all_rows_is_the_default(golden):
    x = golden["sample1500_x"]
    sd = plot.scatter_density(dev(x), max_plot_samples=1000)
    assert sd.idx is None and sd.rows_read == 1500 and np.array_equal(sd.scale, np.amax(x, axis=0))
    assert np.array_equal(sd.sums, dm.kde_sums(x, GRID, GRID, dm.H, sd.scale, sd.shift)[0])


# ---- occupancy counts, bit for bit --------------------------------------------------------------------------------
def counts_dev(x, raster, labels=None, label_lo=0, n_slots=1):
    c, o = engine.density_counts_dev(dev(x), raster, None if labels is None else dev(labels.astype(np.int32)), label_lo,
                                     n_slots)
    return c.cpu().numpy(), int(o.cpu()[0])


@pytest.mark.parametrize("hot_table", [1, 0])
def test_counts_equal_restatement(ppk_option, hot_table):
    ppk_option("density_hot_table", hot_table)
    x = random_rows(70001, 21)
    raster = (-0.05, 67.0, 67, 0.0, 45.5, 41)          # x in [-0.05, 0.95), y in [0, 0.9): part of the rows
    want, outside = dm.counts(x, raster)
    assert outside > 0 and want.sum() + outside == len(x)
    got, got_out = counts_dev(x, raster)
    assert got.dtype == np.uint32 and got.shape == (1, 41, 67) and np.array_equal(got, want) and got_out == outside
    labels = np.random.RandomState(2).randint(-1, 4, size=len(x))
    want, outside = dm.counts(x, raster, labels, -1, 5)
    got, got_out = counts_dev(x, raster, labels, -1, 5)
    assert got.shape == (5, 41, 67) and np.array_equal(got, want) and got_out == outside
    # the host-array twin
    got, got_out = engine.density_counts(x, raster, labels, -1, 5)
    assert np.array_equal(got, want) and got_out == outside


@pytest.mark.parametrize("hot_table", [1, 0])
def test_counts_edges_one_pixel_and_no_rows(ppk_option, hot_table):
    ppk_option("density_hot_table", hot_table)
    raster = (0.25, 8.0, 6, -0.5, 4.0, 8)          # x in [0.25, 1), y in [-0.5, 1.5)
    edge = np.float32(1.0)
    x = np.array([[0.25, -0.5], [edge, 0.0], [np.nextafter(edge, np.float32(0)), 0.0], [np.nextafter(edge, np.float32(2)), 0.0],
                  [np.nextafter(np.float32(0.25), np.float32(0)), 0.0], [0.5, 1.5], [0.5, np.nextafter(np.float32(1.5), np.float32(0))]],
                 dtype=np.float32)
    want, outside = dm.counts(x, raster)
    assert outside == 4 and want[0, 0, 0] == 1 and want[0, 2, 5] == 1 and want[0, 7, 2] == 1
    got, got_out = counts_dev(x, raster)
    assert np.array_equal(got, want) and got_out == outside
    # 200 000 rows in one pixel
    x = np.tile(np.array([[0.6, 0.3]], dtype=np.float32), (200000, 1))
    got, got_out = counts_dev(x, raster)
    assert got_out == 0 and got.sum() == 200000 and got[0, 3, 2] == 200000
    got, got_out = counts_dev(np.zeros((0, 2), dtype=np.float32), raster)
    assert got_out == 0 and got.shape == (1, 8, 6) and not got.any()


def test_counts_at_the_figure_size():
    x = random_rows(250000, 4)
    labels = (x[:, 0] > 0.3).astype(np.int64) + (x[:, 1] > 0.5)
    raster, extent = plot.raster_for(np.amax(x, axis=0))
    assert raster[2] == 1760 and raster[5] == 1280
    want, outside = dm.counts(x, raster, labels, 0, 3)
    got, got_out = counts_dev(x, raster, labels, 0, 3)
    assert outside == 0 and got_out == 0 and got.shape == (3, 1280, 1760) and np.array_equal(got, want)
    c, o, ext = plot.label_raster(dev(x), dev(labels), 0, 3)
    assert np.array_equal(c, want) and o == 0 and ext == extent


# ---- argument errors, by message and by the row they name ---------------------------------------------------------
def test_kde_errors(blobs):
    x, scale, _, _, _ = blobs
    bad = x.copy()
    bad[2100, 1] = np.nan
    bad[400, 0] = np.inf
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: row 400: value \(inf, .*\) is not finite"):
        kde_dev(bad, GRID, GRID, dm.H, scale)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: row 400: value \(inf, .*\) is not finite"):
        kde_dev(bad, GRID, GRID, dm.H, None)
    idx = np.array([5, 2100, 9, 400, 2100])
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: index 1: row 2100: value \(.*, nan\) is not finite"):
        kde_dev(bad, GRID, GRID, dm.H, scale, idx=idx)
    kde_dev(bad, GRID, GRID, dm.H, scale, idx=np.array([5, 9, 2999]))        # rows not read are not looked at
    for k, v in ((3, 3000), (1, -1)):
        idx = np.array([5, 7, 9, 11, 13])
        idx[k] = v
        with pytest.raises(RuntimeError, match=r"ppk_density_kde: index %d: row %d outside \[0, 3000\)" % (k, v)):
            kde_dev(x, GRID, GRID, dm.H, scale, idx=idx)
    for s in ((0.0, 1.0), (1.0, -2.0), (np.nan, 1.0), (1.0, np.inf)):
        with pytest.raises(RuntimeError, match=r"ppk_density_kde: scale\[[01]\] = .* must be finite and positive"):
            kde_dev(x, GRID, GRID, dm.H, s)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: scale\[0\] = 0 \(the column maximum\) must be finite and positive"):
        kde_dev(np.array([[0.0, 1.0], [0.0, 0.5]], dtype=np.float32), GRID, GRID, dm.H, None)
    for h in (0.0, -0.03, np.nan, np.inf):
        with pytest.raises(RuntimeError, match="ppk_density_kde: h = .* must be finite and positive"):
            kde_dev(x, GRID, GRID, h, scale)
    with pytest.raises(RuntimeError, match="ppk_density_kde: gx is not strictly ascending at index 50"):
        g = GRID.copy()
        g[50] = g[49]
        kde_dev(x, g, GRID, dm.H, scale)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: gy\[99\] is not finite"):
        g = GRID.copy()
        g[99] = np.nan
        kde_dev(x, GRID, g, dm.H, scale)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: nx \* ny \+ nx \+ ny must be 1 \.\. 10240 .*100 x 100 fits.*nx = 101, ny = 101"):
        kde_dev(x, np.linspace(0, 1, 101), np.linspace(0, 1, 101), dm.H, scale)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: nx \* ny \+ nx \+ ny must be 1 \.\. 10240"):
        kde_dev(x, np.zeros(0), GRID, dm.H, scale)
    for shift in (-1, 41):
        with pytest.raises(RuntimeError, match="ppk_density_kde: shift must be 0 .. 40"):
            kde_dev(x, GRID, GRID, dm.H, scale, shift=shift)
    with pytest.raises(RuntimeError, match=r"ppk_density_kde: shift must be at most 62 - ceil_log2\(rows read\)"):
        kde_dev(np.zeros(((1 << 22) + 1, 2), dtype=np.float32), [0.0, 1.0], [0.0, 1.0], dm.H, (1, 1), shift=40)
    with pytest.raises(RuntimeError, match="ppk_density_kde: no rows read"):
        kde_dev(x, GRID, GRID, dm.H, None, idx=np.zeros(0, dtype=np.int64))


def test_counts_errors():
    x = random_rows(5000, 9)
    raster = (0.0, 10.0, 32, 0.0, 10.0, 32)
    bad = x.copy()
    bad[4000, 0] = np.nan
    bad[123, 1] = -np.inf
    labels = np.zeros(5000, dtype=np.int64)
    labels[77] = 9                               # a bad label before the bad value: the value is reported first
    with pytest.raises(RuntimeError, match=r"ppk_density_counts: row 123: value \(.*, -inf\) is not finite"):
        counts_dev(bad, raster, labels, 0, 2)
    labels[3000], labels[77] = -2, 1
    labels[4999] = 2
    with pytest.raises(RuntimeError, match=r"ppk_density_counts: row 3000: label -2 outside \[-1, 2\)"):
        counts_dev(x, raster, labels, -1, 3)
    labels[3000] = 0
    with pytest.raises(RuntimeError, match=r"ppk_density_counts: row 4999: label 2 outside \[-1, 2\)"):
        counts_dev(x, raster, labels, -1, 3)
    for r, msg in (((np.inf, 10.0, 32, 0.0, 10.0, 32), "x0 and y0 must be finite"),
                   ((0.0, 10.0, 32, np.nan, 10.0, 32), "x0 and y0 must be finite"),
                   ((0.0, 0.0, 32, 0.0, 10.0, 32), "inv_dx and inv_dy must be finite and positive"),
                   ((0.0, 10.0, 32, 0.0, -1.0, 32), "inv_dx and inv_dy must be finite and positive"),
                   ((0.0, 10.0, 32, 0.0, np.inf, 32), "inv_dx and inv_dy must be finite and positive")):
        with pytest.raises(RuntimeError, match="ppk_density_counts: " + msg):
            counts_dev(x, r)
    lib_args = dict(labels=np.zeros(5000, dtype=np.int64))
    with pytest.raises(RuntimeError, match=r"ppk_density_counts: n_slots \* nx \* ny must be at most 2\^26"):
        counts_dev(x, (0.0, 1.0, 4096, 0.0, 1.0, 4096), n_slots=8, **lib_args)
    with pytest.raises(RuntimeError, match="ppk_density_counts: n_slots must be 1 without labels"):
        counts_dev(x, raster, n_slots=2)
    with pytest.raises(ValueError, match="n_slots must be 1 .. 32 and nx, ny 1 .. 4096"):
        counts_dev(x, (0.0, 1.0, 4097, 0.0, 1.0, 32))


# ---- the plots ----------------------------------------------------------------------------------------------------
class Anything:
    """Stands in for whatever a pyplot call returns."""

    def __getattr__(self, name):
        return Anything()

    def __call__(self, *args, **kwargs):
        return Anything()


class RecordingPlt:
    def __init__(self):
        self.calls = []
        self.cm = Anything()

    def __getattr__(self, name):
        def record(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return Anything()
        return record

    def subplot(self, *args, **kwargs):
        from matplotlib.transforms import Bbox
        self.calls.append(("subplot", args, kwargs))
        axes = Anything()
        axes.bbox = Bbox.unit()             # (Ellipse.set_clip_box takes a real one only)
        return axes

    def names(self):
        return [c[0] for c in self.calls]


def bgmm_of(x):
    """A two-component model over the two blobs, from their own moments."""
    from poppunk_amd.models import BGMMModel
    scale = np.amax(x, axis=0)
    xs = (x / scale).astype(np.float64)
    near = xs[:, 1] < 0.4
    parts = [xs[near], xs[~near]]
    return BGMMModel([len(p) / len(xs) for p in parts], [p.mean(axis=0) for p in parts],
                     [np.cov(p.T) for p in parts], scale, within_label=0, between_label=1)


def draw_all(x_t, y_t, y_refine, model, out, **kw):
    plot.plot_scatter(x_t, out, "Distances", **kw)
    plot.plot_results(x_t, y_t, model.means, model.covariances, model.scale, "BGMM", os.path.join(out, "fit_DPGMM_fit"), **kw)
    mean0, mean1 = np.array([0.1, 0.1]), np.array([0.6, 0.7])
    plot.plot_refined_results(x_t, y_refine, 0.4, 0.5, 0.3, 0.45, mean0, mean1, 0.1, 0.2, model.scale, False, True, False,
                              "Refined fit boundary", os.path.join(out, "fit_refined_fit"), **kw)
    assert mean0.tolist() == [0.1, 0.1] and mean1.tolist() == [0.6, 0.7]       # not scaled in place


def test_plots_write_the_reference_file_names(golden, tmp_path):
    pytest.importorskip("matplotlib")
    import torch
    x = golden["blobs3000_x"]
    model = bgmm_of(x)
    x_t = dev(x)
    y_t = model.assign_dev(x_t)
    y_refine = torch.where(y_t == 0, -1, 1).to(torch.int32)
    out = str(tmp_path / "db")
    os.makedirs(out)
    draw_all(x_t, y_t, y_refine, model, out)
    model.plot(x_t, y_t, outPrefix=out)
    want = {"db_distanceDistribution.png", "fit_DPGMM_fit.png", "fit_refined_fit.png", "db_DPGMM_fit.png",
            "db_DPGMM_fit_contours.pdf"}
    assert want <= set(os.listdir(out))
    assert all(os.path.getsize(os.path.join(out, f)) > 10000 for f in want)


@pytest.mark.parametrize("raster_above,layer", [(1000000, "points"), (0, "raster")])
def test_plots_take_the_scatter_or_the_raster_route(golden, tmp_path, monkeypatch, raster_above, layer):
    pytest.importorskip("matplotlib.pyplot")
    import matplotlib as mpl
    import torch
    rec = RecordingPlt()
    monkeypatch.setattr(plot, "_pyplot", lambda: (mpl, rec))
    x = golden["blobs3000_x"]
    model = bgmm_of(x)
    x_t = dev(x)
    y_t = model.assign_dev(x_t)
    y_refine = torch.where(y_t == 0, -1, 1).to(torch.int32)
    draw_all(x_t, y_t, y_refine, model, str(tmp_path), raster_above=raster_above)
    names = rec.names()
    assert names.count("savefig") == 3 and names.count("close") == 3 and names.count("contour") == 1
    if layer == "points":
        assert names.count("imshow") == 0 and names.count("scatter") == 1 + 2 + 2
        sc = [c for c in rec.calls if c[0] == "scatter"][0]
        assert np.array_equal(sc[1][0], golden["blobs3000_scatter_x"]) and sc[2] == {"s": 1, "alpha": 1}
    else:
        assert names.count("scatter") == 0 and names.count("imshow") == 3
        imgs = [c for c in rec.calls if c[0] == "imshow"]
        assert all(c[1][0].shape == (1280, 1760, 4) and c[2]["origin"] == "lower" for c in imgs)
        # the BGMM picture: every occupied pixel carries the colour of the highest component in it
        counts, _, _ = plot.label_raster(x_t, y_t, 0, 2)
        img = imgs[1][1][0]
        both = (counts[0] > 0) & (counts[1] > 0)
        only0 = (counts[0] > 0) & ~both
        c0, c1 = (np.asarray(mpl.colors.to_rgba(c), dtype=np.float32) for c in plot.BGMM_COLOURS[:2])
        assert only0.any() and np.all(img[only0] == c0) and np.all(img[counts[1] > 0] == c1)
        assert np.all(img[(counts[0] == 0) & (counts[1] == 0)] == 0)
    saved = [c[1][0] for c in rec.calls if c[0] == "savefig"]
    assert saved == [os.path.join(str(tmp_path), os.path.basename(str(tmp_path)) + "_distanceDistribution.png"),
                     os.path.join(str(tmp_path), "fit_DPGMM_fit.png"), os.path.join(str(tmp_path), "fit_refined_fit.png")]
