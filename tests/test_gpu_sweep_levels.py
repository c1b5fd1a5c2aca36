"""ppk_sweep_levels_dev on a real MI355X: the sweep level of listed rows.

Every row of a dense matrix is listed; the rows with a level below n_off, as (i, j, level), must then be what
threshold_iterate_1d_dev / _2d_dev return for the matrix, as sets (sorted).  Boundaries are placed through values that
occur in the matrix, so rows lie on the lines or within a rounding of them."""
import numpy as np
import pytest

from poppunk_amd import engine, synth

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
N_OFFS = (1, 40, 125, 1023)          # 125: the 32-bit candidate words of the matrix side; 1 023: the limit


@pytest.fixture(scope="module")
def matrices():
    sk, _ = synth.make_sketches(300, KMERS, cluster_size=30)
    tbl = synth.random_match_table(KMERS)
    out = {}
    for n in (65, 300):
        db = engine.SketchDB(sk[:n], 16, 14, device=0)
        out[n] = engine.dist(db, None, KMERS, tbl)[0]
        db.close()
    return out


def _keys_of_sweep(i_t, j_t, o_t, n):
    i, j, o = (t.cpu().numpy() for t in (i_t, j_t, o_t))
    rows = i * n - i * (i + 1) // 2 + (j - i - 1)
    return np.sort(rows * 1024 + o)


def _keys_of_levels(level_t, n_off):
    lv = level_t.cpu().numpy().astype(np.int64)
    assert lv.min() >= 0 and lv.max() <= n_off
    rows = np.nonzero(lv < n_off)[0]
    return np.sort(rows * 1024 + lv[rows])


def _line_and_offsets(d, slope, n_off, rng):
    """A sweep line and n_off sorted offsets whose boundaries pass through rows of the matrix."""
    picks = d[rng.choice(d.shape[0], size=n_off, replace=n_off > d.shape[0])].astype(np.float64)
    if slope == 0:          # x_max = (float)offset: the core values themselves
        return (0.0, 0.0, 1.0, 0.0), np.sort(picks[:, 0])
    if slope == 1:          # y_max = (float)offset
        return (0.0, 0.0, 0.0, 1.0), np.sort(picks[:, 1])
    x0, y0 = 0.0, 0.0
    x1, y1 = float(np.quantile(d[:, 0], 0.6)), float(np.quantile(d[:, 1], 0.6))
    ds = np.hypot(x1 - x0, y1 - y0)
    off = ((picks[:, 0] - x0) * (x1 - x0) + (picks[:, 1] - y0) * (y1 - y0)) / ds      # the rows' projections
    return (x0, y0, x1, y1), np.sort(np.maximum(off, 1e-4))


@pytest.mark.parametrize("slope", [0, 1, 2])
@pytest.mark.parametrize("n", [65, 300])
def test_levels_equal_the_1d_sweep(n, slope, matrices, ppk_option):
    dist_t = matrices[n]
    d = dist_t.cpu().numpy()
    rng = np.random.default_rng(10 * n + slope)
    for n_off in N_OFFS:
        line, offsets = _line_and_offsets(d, slope, n_off, rng)
        x_max, y_max = engine.sweep_boundaries_1d(offsets, slope, *line)
        level = engine.sweep_levels_dev(dist_t, x_max, y_max, slope)
        got = _keys_of_levels(level, n_off)
        assert 0 < got.size, (n_off,)
        for window in (0, 1):
            ppk_option("sweep_window", window)
            want = _keys_of_sweep(*engine.threshold_iterate_1d_dev(dist_t, offsets, slope, *line), n)
            assert np.array_equal(got, want), (n_off, window)


@pytest.mark.parametrize("n", [65, 300])
def test_levels_equal_the_2d_sweep(n, matrices, ppk_option):
    dist_t = matrices[n]
    d = dist_t.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(n)
    y_max = float(np.quantile(d[:, 1], 0.9))
    for n_off in N_OFFS:
        # x_max such that a picked row lies on the line x / x_max + y / y_max = 1
        picks = d[rng.choice(d.shape[0], size=4 * n_off)]
        picks = picks[(picks[:, 1] < 0.8 * y_max) & (picks[:, 0] > 0)][:n_off]
        assert picks.shape[0] == n_off
        x_max = np.sort((picks[:, 0] / (1.0 - picks[:, 1] / y_max)).astype(np.float32))
        assert x_max[0] > 0
        level = engine.sweep_levels_dev(dist_t, x_max, np.full(n_off, y_max, dtype=np.float32), 2)
        got = _keys_of_levels(level, n_off)
        assert got.size > 0
        for window in (0, 1):
            ppk_option("sweep_window", window)
            want = _keys_of_sweep(*engine.threshold_iterate_2d_dev(dist_t, x_max, y_max), n)
            assert np.array_equal(got, want), (n_off, window)


def test_small_lists_and_alignment(matrices):
    import torch
    dist_t = matrices[65]
    d = dist_t.cpu().numpy()
    x_max = np.sort(d[::50, 0]).astype(np.float32) + np.float32(1e-3)
    y_max = np.sort(d[::50, 1]).astype(np.float32) + np.float32(1e-3)
    n_off = x_max.size
    for slope in (0, 1, 2):
        whole = engine.sweep_levels_dev(dist_t, x_max, y_max, slope)
        # no rows, one row
        none = engine.sweep_levels_dev(dist_t[:0].contiguous(), x_max, y_max, slope)
        assert none.shape == (0,) and none.dtype == torch.int32
        one = engine.sweep_levels_dev(dist_t[7:8].contiguous(), x_max, y_max, slope)
        assert torch.equal(one, whole[7:8])
        # a list that starts 4 bytes off an 8-byte boundary
        flat = torch.empty(2 * dist_t.shape[0] + 1, dtype=torch.float32, device=dist_t.device)
        odd = flat[1:].view(-1, 2)
        odd.copy_(dist_t)
        assert odd.data_ptr() % 8 == 4
        assert torch.equal(engine.sweep_levels_dev(odd, x_max, y_max, slope), whole)
        # any order of rows: the level belongs to the coordinates
        perm = torch.randperm(dist_t.shape[0], device=dist_t.device, generator=torch.Generator(dist_t.device).manual_seed(1))
        assert torch.equal(engine.sweep_levels_dev(dist_t[perm].contiguous(), x_max, y_max, slope), whole[perm])
        # a slope-2 boundary on an axis (ppk_line_dist's sqrt branch), NaN rows, no boundary at all
        if slope == 2:
            xz = x_max.copy()
            xz[0] = 0.0
            lv = engine.sweep_levels_dev(dist_t, xz, y_max, slope)
            a0 = engine.assign_threshold_dev(dist_t, 2, 0.0, float(y_max[0]))
            assert torch.equal(lv == 0, a0 <= 0)
        bad = dist_t.clone()
        bad[3, 0] = float("nan")
        assert int(engine.sweep_levels_dev(bad, x_max, y_max, slope)[3].item()) == (n_off if slope != 1 else int(whole[3].item()))
    with pytest.raises(RuntimeError, match="1023"):
        engine.sweep_levels_dev(dist_t, np.zeros(1024, np.float32), np.zeros(1024, np.float32), 2)
    # the level of a row is the first boundary that assign_threshold_dev puts it within
    first = torch.full((dist_t.shape[0],), n_off, dtype=torch.int32, device=dist_t.device)
    for o in reversed(range(n_off)):
        within = engine.assign_threshold_dev(dist_t, 2, float(x_max[o]), float(y_max[o])) <= 0
        first[within] = o
    assert torch.equal(engine.sweep_levels_dev(dist_t, x_max, y_max, 2), first)
