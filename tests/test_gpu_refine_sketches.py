"""The refine fit from resident sketches on a real MI355X (refine.SketchScorer, RefineBoundary.fit_from_sketches;
DESIGN.md 3.26).

The matrix route is the yardstick: refine.DeviceScorer and RefineBoundary.fit_dev on engine.dist(db) of the same
database.  Scores, counts, evaluation sequences and fitted values must come out equal, not close."""
import numpy as np
import pytest

from poppunk_amd import engine, models, refine, synth

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)


def _same_list(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:          # (the comparison is of the errors themselves)
        return ("error", type(e).__name__, str(e))


@pytest.fixture(scope="module")
def pop300():
    import torch
    sk, _ = synth.make_sketches(300, KMERS, cluster_size=30)
    tbl = synth.random_match_table(KMERS)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dense, _ = engine.dist(db, None, KMERS, tbl)
    scale = dense.max(dim=0).values.cpu().numpy().astype(np.float32)
    scaled = dense / torch.as_tensor(scale, device=dense.device)
    d = scaled.cpu().numpy().astype(np.float64)
    close = d[:, 0] < np.quantile(d[:, 0], 0.1)
    return {"db": db, "tbl": tbl, "scale": scale, "scaled": scaled, "mean0": d[close].mean(axis=0),
            "mean1": d[~close].mean(axis=0)}


def _scorers(p):
    return refine.SketchScorer(p["db"], KMERS, p["tbl"], p["scale"]), refine.DeviceScorer(p["scaled"])


def test_scorer_sweeps_scores_and_cache(pop300):
    p = pop300
    sk_s, dev_s = _scorers(p)
    assert sk_s.n_rows == dev_s.n_rows == 300 * 299 // 2
    m0, m1 = p["mean0"], p["mean1"]
    length = float(np.hypot(*(m1 - m0)))
    s_range = np.linspace(0.0, 0.6 * length, 40)
    for slope in (2, 0, 1):
        for score_idx in (0, 1):
            got = sk_s.sweep_1d(s_range, slope, m0, m1, score_idx)
            want = dev_s.sweep_1d(s_range, slope, m0, m1, score_idx)
            assert got[0] == want[0] and 0 < got[0] < sk_s.n_rows, (score_idx, slope)
            assert _same_list(got[1], want[1]), (score_idx, slope)
    # one pass per slope: the second score of a slope was served from the list the first one made
    assert sk_s.passes == 3
    # inside the kept list (slope 1, the last sweep): no pass; outside it: one more
    gradient = (m1[1] - m0[1]) / (m1[0] - m0[0])
    before = sk_s.passes
    for s in (0.1 * length, 0.3 * length, 0.55 * length):
        x, y = refine.boundary_of_s(s, m0, m1, gradient, 1)
        for score_idx in (0, 1):
            got, want = sk_s.score(1, x, y, score_idx), dev_s.score(1, x, y, score_idx)
            assert np.array_equal(np.asarray(got[0]).ravel(), np.asarray(want[0]).ravel()), (s, score_idx)
            assert (got[1] is None and want[1] is None) or _same_list(got[1], want[1])
    assert sk_s.passes == before
    for k, s in enumerate((0.7 * length, 0.9 * length)):
        x, y = refine.boundary_of_s(s, m0, m1, gradient, 2)
        got, want = sk_s.score(2, x, y, 0), dev_s.score(2, x, y, 0)
        assert np.array_equal(got[0], want[0]) and got[0][0] > 0
    assert sk_s.passes == before + 2          # another slope, then a line outside that list
    x, y = refine.boundary_of_s(0.4 * length, m0, m1, gradient, 2)
    assert np.array_equal(sk_s.score(2, x, y, 0)[0], dev_s.score(2, x, y, 0)[0]) and sk_s.passes == before + 2
    # a slope-2 line on an axis (line_dist's sqrt branch): a pass of its own, and nothing is kept of it
    for x, y in ((0.0, 0.3), (0.2, 0.0)):
        assert np.array_equal(sk_s.score(2, x, y, 0)[0], dev_s.score(2, x, y, 0)[0])
    assert sk_s.passes == before + 4
    x, y = refine.boundary_of_s(0.5 * length, m0, m1, gradient, 2)
    assert np.array_equal(sk_s.score(2, x, y, 0)[0], dev_s.score(2, x, y, 0)[0]) and sk_s.passes == before + 4
    # the 2-D sweep, one y at a time: the first y makes the list, smaller ones read it
    x_range = np.linspace(0.05, 0.5, 20, dtype=np.float32)
    for y_max in (np.float32(0.5), np.float32(0.3), np.float32(0.1)):
        got, want = sk_s.sweep_2d(x_range, y_max, 0), dev_s.sweep_2d(x_range, y_max, 0)
        assert got[0] == want[0] and _same_list(got[1], want[1]), y_max
    got, want = sk_s.sweep_2d(x_range, np.float32(0.3), 1), dev_s.sweep_2d(x_range, np.float32(0.3), 1)
    assert got[0] == want[0] and _same_list(got[1], want[1])


def test_bracket_and_empty_sweeps(pop300):
    p = pop300
    sk_s, dev_s = _scorers(p)
    m0, m1 = p["mean0"], p["mean1"]
    length = float(np.hypot(*(m1 - m0)))
    gradient = (m1[1] - m0[1]) / (m1[0] - m0[0])
    for slope in (2, 0, 1):
        lo = [np.float32(v) for v in refine.boundary_of_s(0.2 * length, m0, m1, gradient, slope)]
        hi = [np.float32(v) for v in refine.boundary_of_s(0.5 * length, m0, m1, gradient, slope)]
        with dev_s.bracket(slope, lo, hi) as want_h:
            got_h = sk_s.bracket(slope, lo, hi)
            assert got_h is not None and sum(got_h.split) == sk_s.n_rows
            for s in (0.2, 0.27, 0.333, 0.41, 0.5):
                x, y = refine.boundary_of_s(s * length, m0, m1, gradient, slope)
                assert np.array_equal(got_h.eval(x, y), want_h.eval(x, y)), (slope, s)
            got_h.close()
        # not nested: no handle, on either route
        assert sk_s.bracket(slope, hi, lo) is None and dev_s.bracket(slope, hi, lo) is None
    assert sk_s.bracket(2, [0.0, 0.1], [0.2, 0.3]) is None and dev_s.bracket(2, [0.0, 0.1], [0.2, 0.3]) is None
    # a sweep that lists nothing: the reference's message, from either route
    tiny = np.linspace(0.0, 1e-7, 5)
    a0, a1 = np.array([1e-7, 1e-7]), np.array([2e-7, 2e-7])
    for slope in (2, 0):
        got = _outcome(lambda: sk_s.sweep_1d(tiny, slope, a0, a1, 0))
        want = _outcome(lambda: dev_s.sweep_1d(tiny, slope, a0, a1, 0))
        assert want[0] == "error" and got == want
    got = _outcome(lambda: sk_s.sweep_2d(np.float32([1e-7, 2e-7]), np.float32(1e-7), 0))
    want = _outcome(lambda: dev_s.sweep_2d(np.float32([1e-7, 2e-7]), np.float32(1e-7), 0))
    assert want[0] == "error" and got == want
    with pytest.raises(NotImplementedError):
        models.RefineBoundary().fit_from_sketches(p["db"], KMERS, p["tbl"], [], None, 0.0, 0.0, sample_size=10)


@pytest.fixture(scope="module")
def fit240():
    """tests/test_gpu_refine_fit.py::test_model_fit_after_bgmm's population and start model."""
    sk, _ = synth.make_sketches(240, KMERS, cluster_size=20, seed=7)
    tbl = synth.random_match_table(KMERS)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, KMERS, tbl)
    bgmm = models.BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    return {"db": db, "tbl": tbl, "dist": dist_t, "bgmm": bgmm, "names": ["g%d" % k for k in range(240)]}


@pytest.fixture
def fit_records(monkeypatch):
    """Every refine.refineFit call from here on leaves (slope, global scores, bounds, evaluations, outcome) in a list:
    a fit with indiv_refine makes three calls, and last_fit only keeps the latest."""
    records = []
    real = refine.refineFit

    def recording(*args, **kw):
        out = _outcome(lambda: real(*args, **kw))
        info = refine.last_fit
        records.append((kw.get("slope", 2), np.array(info["global_s"], dtype=np.float64), info["bounds"],
                        list(info["evals"]), info["local_path"], out[:1] + out[2:] if out[0] == "error" else out))
        if out[0] == "error":
            raise RuntimeError(out[2])
        return out[1]

    monkeypatch.setattr(refine, "refineFit", recording)
    return records


FITS = {
    "default": ({}, 1),
    "indiv_both": ({"indiv_refine": "both"}, 1),
    "unconstrained": ({"unconstrained": True}, 1),
    "no_local": ({"no_local": True}, 1),
    "refine_local_0": ({"indiv_refine": "both"}, 0),
}


@pytest.mark.parametrize("case", sorted(FITS))
def test_fit_from_sketches_equals_fit_dev(case, fit240, ppk_option, fit_records):
    import torch
    kw, local = FITS[case]
    ppk_option("refine_local", local)
    f = fit240
    want = models.RefineBoundary()
    y = want.fit_dev(f["dist"], f["names"], f["bgmm"], 0.0, 0.0, **kw)
    want_recs = list(fit_records)
    del fit_records[:]
    got = models.RefineBoundary()
    edges, n_failed = got.fit_from_sketches(f["db"], KMERS, f["tbl"], f["names"], f["bgmm"], 0.0, 0.0, **kw)
    got_recs = list(fit_records)
    for name in ("optimal_x", "optimal_y", "optimal_s", "core_boundary", "accessory_boundary"):
        assert float(getattr(got, name)) == float(getattr(want, name)), name
    assert (got.fitted, got.indiv_fitted, got.slope, got.unconstrained) == \
        (want.fitted, want.indiv_fitted, want.slope, want.unconstrained)
    assert np.array_equal(got.scale, want.scale) and np.array_equal(got.mean0, want.mean0)
    # every refineFit call of either fit: the same slope, global scores, bounds, evaluations (positions, counts,
    # scores), in the same order, with the same outcome
    assert len(got_recs) == len(want_recs) == (3 if kw.get("indiv_refine") == "both" else 1)
    for got_rec, want_rec in zip(got_recs, want_recs):
        assert got_rec[0] == want_rec[0]
        assert _same_list(got_rec[1], want_rec[1])
        assert got_rec[2] == want_rec[2]
        assert len(got_rec[3]) == len(want_rec[3])
        for a, b in zip(got_rec[3], want_rec[3]):
            assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2])))
        assert got_rec[4] == want_rec[4]          # the bracket handle served both, or neither
        assert repr(got_rec[5]) == repr(want_rec[5])
    if case == "default":
        assert len(got_recs[0][3]) > 0          # a local search ran, and was compared
    want_edges = engine.generate_tuples_dev(y.to(torch.int32), want.within_label, True)
    assert want_edges.shape[0] > 0 and torch.equal(edges, want_edges)
    assert int(n_failed.item()) == 0
    # a handful of passes over the sketches, not one per evaluation
    assert 1 <= got.fit_passes <= 6, got.fit_passes
