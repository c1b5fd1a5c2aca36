"""GPU tests of the refine fit (ppk_refine_score_dev, ppk_refine_local_*, refine.refineFit, models.RefineBoundary.fit;
DESIGN.md 3.14): one boundary's counts against edge_threshold_dev + network_sweep_dev, the bracket handle against the
one-boundary call on every kind of split, and the fit against the reference's own steps
(tests/golden/refine_fit.npz).  The bar of the trajectory comparison is exact equality: the host check of the same
golden (tests/test_refine_fit_host.py) reproduces every position, score and result exactly."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, models, refine, utils  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def clustered_distances(n, n_clusters, seed):
    """condensed float32 [n(n-1)/2, 2] scaled to [0, 1]: short distances inside a cluster, longer ones between"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, n_clusters, n)
    ii, jj = np.triu_indices(n, 1)
    same = lab[ii] == lab[jj]
    core = np.where(same, rng.uniform(0.0, 0.02, ii.size), rng.uniform(0.01, 0.05, ii.size))
    acc = core * rng.uniform(2.0, 4.0, ii.size) + rng.uniform(0.0, 0.02, ii.size)
    d = np.stack([core, acc], axis=1)
    return (d / d.max(axis=0)).astype(np.float32)


LO, HI, MID = (0.375, 0.5), (0.625, 0.75), (0.5, 0.5)      # dyadic: x_max * y_max and the planted sums are exact


def planted(d, seed):
    """rows exactly on LO, MID and HI, within 2^-20 of them (relatively) on both sides, a row at the origin, and rows
    with a NaN and with a negative coordinate, scattered over the matrix"""
    d = d.copy()
    rows = []
    for xm, ym in (LO, MID, HI):
        on = [(xm / 2, ym / 2), (xm, 0.0), (0.0, ym), (xm / 4, 3 * ym / 4)]
        rows += on
        for x, y in on[:2]:
            for f in (1 + 2.0**-21, 1 - 2.0**-21, 1 + 2.0**-19, 1 - 2.0**-19):
                rows.append((np.float32(x) * np.float32(f), y))
            rows.append((np.nextafter(np.float32(x), np.float32(1)), y))
            rows.append((np.nextafter(np.float32(x), np.float32(0)), y))
    rows += [(0.0, 0.0), (np.nan, 0.1), (0.1, np.nan), (np.nan, np.nan), (-0.1, 0.2), (0.2, -0.1), (-0.3, -0.3)]
    at = np.random.default_rng(seed).choice(d.shape[0], size=len(rows), replace=False)
    d[at] = np.array(rows, dtype=np.float32)
    return d


@pytest.fixture(scope="module")
def mats():
    out = {}
    for n, k, seed in ((301, 12, 1), (64, 4, 2)):
        plain = clustered_distances(n, k, seed)
        out[n] = {"plain": plain, "planted": planted(plain, seed)}
        out[n].update({k + "_t": torch.from_numpy(v).to(DEV) for k, v in list(out[n].items())})
    return out


def yardstick(dist_t, n, slope, x, y):
    """the parent's path: the edge list of one boundary, then the sweep's counts at one offset"""
    e = engine.edge_threshold_dev(dist_t, slope, x, y)
    return engine.network_stats_dev(e, n)[0].cpu().numpy()


SCORE_LINES = [(2, 0.5, 0.5), (2, 0.3, 0.7), (2, 0.05, 0.9), (2, 1.5, 1.5), (2, 0.01, 0.01), (2, 0.4, 0.0), (2, 0.0, 0.4),
               (0, 0.5, 0.0), (0, 0.2, 0.0), (0, 0.0, 0.0), (1, 0.0, 0.5), (1, 0.0, 0.15), (1, 0.0, 2.0)]


@pytest.mark.parametrize("n", [301, 64])
def test_score_equals_edge_threshold_and_sweep(mats, n):
    d, t = mats[n]["planted"], mats[n]["planted_t"]
    seen = set()
    for slope, x, y in SCORE_LINES:
        want = yardstick(t, n, slope, x, y)
        got = engine.refine_score_dev(t, slope, x, y)
        assert np.array_equal(got, want), (slope, x, y, got, want)
        assert np.array_equal(engine.refine_score(d, slope, x, y), want)      # host arrays
        seen.add(int(want[0]))
    assert len(seen) > 6 and 1 in seen            # the sqrt branch (an intercept of 0) keeps the row at the origin alone


@pytest.mark.parametrize("n", [2, 3, 65, 129])
def test_score_small_and_word_boundary_sizes(n):
    d = clustered_distances(n, 3, n)
    t = torch.from_numpy(d).to(DEV)
    for slope, x, y in ((2, 0.5, 0.5), (2, 5.0, 5.0), (0, 0.3, 0.0), (2, 1e-6, 1e-6)):
        assert np.array_equal(engine.refine_score_dev(t, slope, x, y), yardstick(t, n, slope, x, y))


def test_score_argument_errors(mats):
    t = mats[64]["plain_t"]
    with pytest.raises(RuntimeError, match="n\\(n-1\\)/2"):
        engine.refine_score_dev(t[:100].contiguous(), 2, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="slope"):
        engine.refine_score_dev(t, 3, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="NaN"):
        engine.refine_score_dev(t, 2, float("nan"), 0.5)


def lines_inside(slope, lo, hi, seed, count=25):
    rng = np.random.default_rng(seed)
    xs, ys = rng.uniform(lo[0], hi[0], count), rng.uniform(lo[1], hi[1], count)
    lines = [lo, hi] + list(zip(xs.tolist(), ys.tolist()))
    if slope == 2:
        lines += [MID, (lo[0], hi[1]), (hi[0], lo[1])]
    return lines


@pytest.mark.parametrize("n", [301, 64])
@pytest.mark.parametrize("slope", [2, 0, 1])
def test_bracket_equals_score(mats, n, slope):
    """25 random lines inside the bracket, both ends and the planted line: rows on an evaluated line and within 2^-20
    of it on both sides, NaN and negative coordinates"""
    t = mats[n]["planted_t"]
    with engine.RefineLocal.create(t, slope, LO[0], LO[1], HI[0], HI[1]) as h:
        base, cand, never = h.split
        print("n", n, "slope", slope, "base / candidates / never", h.split)
        assert base + cand + never == t.shape[0] and base > 0 and cand > 0 and never > 0
        if slope == 2:
            assert cand >= 7 + 3 * 4      # the NaN / negative rows and the rows on the two ends at least
        for x, y in lines_inside(slope, LO, HI, n + slope):
            want = engine.refine_score_dev(t, slope, x, y)
            got = h.eval(x, y)
            assert np.array_equal(got, want), (x, y, got, want)
        assert np.array_equal(h.eval(*MID), yardstick(t, n, slope, *MID))


@pytest.mark.parametrize("n", [301, 64])
def test_bracket_extreme_splits(mats, n):
    t, d = mats[n]["plain_t"], mats[n]["plain"]
    rows = t.shape[0]
    # a bracket of one line that no row is near: no candidates
    x, y = 0.3337, 0.4113
    a = d[:, 1] * np.float32(x) + d[:, 0] * np.float32(y)
    c = np.float32(x) * np.float32(y)
    assert not np.any((a >= c * np.float32(1 - 2.0**-20)) & (a <= c * np.float32(1 + 2.0**-20)))
    with engine.RefineLocal.create(t, 2, x, y, x, y) as h:
        assert h.split[1] == 0 and h.split[0] + h.split[2] == rows
        assert np.array_equal(h.eval(x, y), engine.refine_score_dev(t, 2, x, y))
    # lo so small that the base is empty; hi beyond every row: every row a candidate
    tiny = 2.0**-40
    with engine.RefineLocal.create(t, 2, tiny, tiny, 10.0, 10.0) as h:
        assert h.split == (0, rows, 0)
        for x, y in ((tiny, tiny), (10.0, 10.0), (0.5, 0.5), (0.2, 0.9), (1e-3, 5.0)):
            assert np.array_equal(h.eval(x, y), engine.refine_score_dev(t, 2, x, y)), (x, y)
    with engine.RefineLocal.create(t, 2, tiny, tiny, 0.4, 0.4) as h:
        assert h.split[0] == 0 and h.split[2] > 0
        assert np.array_equal(h.eval(0.3, 0.35), engine.refine_score_dev(t, 2, 0.3, 0.35))
    with engine.RefineLocal.create(t, 2, 0.4, 0.4, 10.0, 10.0) as h:
        assert h.split[2] == 0 and h.split[0] > 0
        assert np.array_equal(h.eval(0.7, 2.0), engine.refine_score_dev(t, 2, 0.7, 2.0))
    # every row in the base
    with engine.RefineLocal.create(t, 0, 5.0, 0.0, 6.0, 0.0) as h:
        assert h.split == (rows, 0, 0)
        assert np.array_equal(h.eval(5.5, 0.0), engine.refine_score_dev(t, 0, 5.5, 0.0))


def test_bracket_evaluations_leave_the_handle_alone(mats):
    t = mats[301]["planted_t"]
    with engine.RefineLocal.create(t, 2, LO[0], LO[1], HI[0], HI[1]) as h:
        first = h.eval(0.45, 0.6)
        other = h.eval(0.6, 0.7)
        again = h.eval(0.45, 0.6)
        assert np.array_equal(first, again) and not np.array_equal(first, other)
        assert np.array_equal(h.eval(*LO), engine.refine_score_dev(t, 2, *LO))      # after larger graphs: still the base
        # a line outside the bracket is an argument error, componentwise
        for x, y in ((0.37, 0.6), (0.63, 0.6), (0.5, 0.49), (0.5, 0.76), (float("nan"), 0.6)):
            with pytest.raises(RuntimeError, match=r"\(1\).*outside the bracket"):
                h.eval(x, y)
        assert np.array_equal(h.eval(0.45, 0.6), first)
    with pytest.raises(RuntimeError, match="closed"):
        h.eval(0.45, 0.6)


def test_not_nested_is_a_status_of_its_own(mats):
    t = mats[64]["plain_t"]
    lib = _lib.lib()
    import ctypes as C
    for slope, lo, hi in ((2, (0.5, 0.5), (0.6, 0.4)), (2, (0.5, 0.5), (0.4, 0.6)), (0, (0.5, 0.0), (0.4, 9.0)),
                          (1, (0.0, 0.5), (9.0, 0.4)), (2, (0.0, 0.5), (0.5, 0.6)), (2, (0.5, 0.5), (float("inf"), 0.6))):
        assert engine.RefineLocal.create(t, slope, lo[0], lo[1], hi[0], hi[1]) is None
        h = C.c_void_p()
        rc = lib.ppk_refine_local_create_dev(C.c_void_p(t.data_ptr()), t.shape[0], slope, lo[0], lo[1], hi[0], hi[1],
                                             None, C.byref(h))
        assert rc == _lib.REFINE_NOT_NESTED == 6 and not h.value and "not nested" in _lib.last_error()
    # slope 0 reads only the x pair, slope 1 only the y pair
    for slope, lo, hi in ((0, (0.4, 9.0), (0.5, 0.0)), (1, (9.0, 0.4), (0.0, 0.5))):
        with engine.RefineLocal.create(t, slope, lo[0], lo[1], hi[0], hi[1]) as h:
            assert sum(h.split) == t.shape[0]


# ---- the fit against the reference's own steps -------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "refine_fit.npz")) as z:
        g = {k: z[k] for k in z.files}
    with np.load(os.path.join(HERE, "golden", "network_sweep.npz")) as z:
        for key in ("sweep1d_dist", "sweep2d_dist"):
            d = z[key]
            g[key] = (d / np.amax(d, axis=0)).astype(np.float32)          # as the generator scaled them
            g[key + "_t"] = torch.from_numpy(g[key]).to(DEV)
    return g


def case_of(g, name):
    pre = name + "_"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def run_fit(g, c, dist, **kw):
    n = {"sweep1d_dist": 300, "sweep2d_dist": 200}[str(c["dist"])]
    res = refine.refineFit(dist, ["s%d" % k for k in range(n)], c["mean0"].copy(), c["mean1"].copy(), c["scale"],
                           float(c["max_move"]), float(c["min_move"]), slope=int(c["slope"]),
                           unconstrained=bool(c["unconstrained"]), no_local=bool(c["no_local"]), **kw)
    return np.array([float(v) for v in res]), refine.last_fit


FIT_CASES = ["slope2_local", "slope0_local", "slope1_local", "slope2_b_local", "unconstrained_local", "no_local",
             "min_at_end", "unconstrained_edge"]


@pytest.mark.parametrize("name", FIT_CASES)
def test_fit_walks_the_reference_trajectory(golden, ppk_option, name):
    """From a resident tensor and from numpy, with the bracket handle and without: the global scores, every position
    the local search evaluates, the four counts and the score of each, and the returned triple equal the reference's
    (exact equality: the bar the host check of the same golden sets)."""
    c = case_of(golden, name)
    key = str(c["dist"])
    paths = []
    for local, dist in ((1, golden[key + "_t"]), (1, golden[key]), (0, golden[key + "_t"])):
        ppk_option("refine_local", local)
        res, info = run_fit(golden, c, dist)
        assert np.array_equal(info["global_s"], c["global_s"])
        assert np.array_equal(np.array([e[0] for e in info["evals"]]), c["eval_s"])
        assert [e[1] for e in info["evals"]] == c["eval_stats"].tolist()
        assert np.array_equal(np.array([e[2] for e in info["evals"]]), c["eval_score"])
        assert (info["bounds"] or []) == c["bounds"].tolist()
        assert np.array_equal(res, c["result"])
        paths.append(info["local_path"])
        if local == 0:
            assert info["local_path"] in (None, "score")
    print(name, "local path", paths, "split", info["split"])
    if name in ("slope2_local", "slope0_local", "slope1_local", "slope2_b_local"):
        assert paths == ["bracket", "bracket", "score"]      # a search direction with positive components is nested


@pytest.mark.parametrize("name", ["below_zero", "all_points"])
def test_fit_errors(golden, name):
    c = case_of(golden, name)
    with pytest.raises(RuntimeError) as e:
        run_fit(golden, c, golden[str(c["dist"]) + "_t"])
    assert str(e.value) == str(c["error"])


def test_fallback_when_the_search_runs_inwards(golden):
    """The line of slope2_local walked from the other end: s grows towards the origin, the two lines of the bounds are
    not nested, and the local search scores through ppk_refine_score_dev -- the same graphs, so the same minimum."""
    import scipy.optimize
    c = case_of(golden, "slope2_local")
    t = golden["sweep1d_dist_t"]
    m0, m1 = c["mean0"], c["mean1"]
    length = float(np.hypot(*(m1 - m0)))
    g = (m1[1] - m0[1]) / (m1[0] - m0[0])
    bounds = [length - c["bounds"][1], length - c["bounds"][0]]
    evals, info = [], {}
    objective, handle = refine._local_objective(refine.DeviceScorer(t), 300, m1, m0, g, 2, 0, bounds, evals, info)
    assert handle is None and info["local_path"] == "score"
    out = scipy.optimize.minimize_scalar(objective, bounds=bounds, method="Bounded")
    assert len(evals) >= 5
    for s, stats, score in evals:
        x, y = refine.boundary_of_s(s, m1, m0, g, 2)
        assert stats == yardstick(t, 300, 2, x, y).tolist()
    assert out.fun in [e[2] for e in evals] and bounds[0] < out.x < bounds[1]


def test_model_fit_after_bgmm(tmp_path, ppk_option):
    """BGMMModel.fit -> RefineBoundary.fit on the 240-genome synthetic database: the 2-D fit and both 1-D fits end to
    end, from a host array and from a resident tensor, saved and loaded."""
    from poppunk_amd import synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(240, kmers, cluster_size=20, seed=7)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    X = dist_t.cpu().numpy()
    names = ["g%d" % k for k in range(240)]
    bgmm = models.BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    means_before = bgmm.means.copy()
    fits = []
    for local, host in ((1, False), (1, True), (0, False)):
        ppk_option("refine_local", local)
        b = models.RefineBoundary()
        if host:
            y = b.fit(X, names, bgmm, 0.0, 0.0, indiv_refine="both")
        else:
            y = b.fit_dev(dist_t, names, bgmm, 0.0, 0.0, indiv_refine="both").cpu().numpy()
        fits.append((b, y))
    b, y = fits[0]
    print("2-D", b.optimal_x, b.optimal_y, "core", b.core_boundary, "accessory", b.accessory_boundary)
    assert b.fitted and b.indiv_fitted is True and b.slope == 2
    assert b.optimal_x > 0 and b.optimal_y > 0 and b.core_boundary > 0 and b.accessory_boundary > 0
    assert b.core_boundary != b.optimal_x and b.accessory_boundary != b.optimal_y      # both 1-D fits filled theirs
    assert np.array_equal(bgmm.means, means_before)
    for other, oy in fits[1:]:
        assert (other.optimal_x, other.optimal_y, other.core_boundary, other.accessory_boundary) == \
            (b.optimal_x, b.optimal_y, b.core_boundary, b.accessory_boundary)
        assert np.array_equal(oy, y) and np.array_equal(other.scale, b.scale)
    assert np.array_equal(y, b.assign(X)) and set(np.unique(y)) <= {-1.0, 0.0, 1.0} and (y == -1).any() and (y == 1).any()
    loaded = models.RefineBoundary.from_npz(b.save(tmp_path / "refined"))
    assert loaded.indiv_fitted is True and np.array_equal(loaded.assign(X), y)
    for slope in (0, 1):
        assert np.array_equal(loaded.assign(X, slope=slope), b.assign(X, slope=slope))
    # a manual start file in place of the model's means: the same start, the same 2-D fit
    start = tmp_path / "start.txt"
    start.write_text("start %r,%r\nend %r,%r\n" % (*means_before[bgmm.within_label].tolist(),
                                                 *means_before[bgmm.between_label].tolist()))
    m = models.RefineBoundary()
    m.fit_dev(dist_t, names, bgmm, 0.0, 0.0, startFile=str(start))
    assert (m.optimal_x, m.optimal_y) == (b.optimal_x, b.optimal_y) and m.indiv_fitted is False
    assert m.core_boundary == m.optimal_x and m.accessory_boundary == m.optimal_y


def test_betweenness_scores_take_the_summary_path(mats):
    n = 64
    t = mats[n]["plain_t"]
    names = ["s%d" % k for k in range(n)]
    m0, m1 = np.array([0.05, 0.05]), np.array([0.6, 0.6])
    for score_idx in (1, 2):
        for s in (0.05, 0.2, 0.4):
            got = refine.newNetwork(s, names, t, m0, m1, 1.0, score_idx=score_idx)
            x, y = refine.boundary_of_s(s, m0, m1, 1.0, 2)
            st, bt, _, _ = engine.network_summary_graph_dev(engine.edge_threshold_dev(t, 2, x, y), n)
            want = -refine.summary_from_stats(st.cpu().numpy(), n, bt.cpu().numpy())[1][score_idx]
            assert got == want or (np.isnan(got) and np.isnan(want))
    res = refine.refineFit(t, names, m0.copy(), m1.copy(), np.array([1.0, 1.0]), 0.0, 0.0, score_idx=1)
    info = refine.last_fit
    offs = np.linspace(0.0, float(np.hypot(*(m1 - m0))), 40)
    want = np.array(engine.refine_sweep_scores_dev(t, offs, 2, m0[0], m0[1], m1[0], m1[1], score_idx=1)[1])
    want[np.isnan(want)] = 1
    assert np.array_equal(info["global_s"], want)
    assert info["local_path"] in (None, "summary") and len(res) == 3
    if info["local_path"] == "summary":
        for s, stats, score in info["evals"]:
            assert score == refine.newNetwork(s, names, t, m0, m1, 1.0, score_idx=1)
