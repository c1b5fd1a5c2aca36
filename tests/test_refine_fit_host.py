"""CPU tests of the refine fit's host side (poppunk_amd/refine.py, utils.py, models.RefineBoundary)
against tests/golden/refine_fit.npz, which holds what the reference's own refineFit did step by step
(tests/golden/make_golden_refine_fit.py).  No device: refineFit is driven by a stand-in for refine.DeviceScorer that
replays recorded score lists and counts."""
import os

import numpy as np
import pytest

from poppunk_amd import models, refine, utils

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_fit.npz")
SWEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "network_sweep.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_of(g, name):
    pre = name + "_"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def n_of(c):
    return {"sweep1d_dist": 300, "sweep2d_dist": 200}[str(c["dist"])]


class Replay:
    """refine.DeviceScorer's methods from recorded data: the sweeps return the recorded global scores (`listed` rows
    listed), every evaluation the next recorded counts.  No `bracket`: the local search scores one boundary at a time."""

    def __init__(self, n, global_s, eval_stats=(), listed=0):
        self.n_rows = n * (n - 1) // 2
        self.global_s, self.eval_stats, self.listed = np.asarray(global_s, dtype=np.float64), list(eval_stats), listed
        self.calls_2d, self.lines = 0, []

    def sweep_1d(self, s_range, slope, mean0, mean1, score_idx):
        self.s_range = np.array(s_range)
        return self.listed, list(self.global_s)

    def sweep_2d(self, x_range, y_max, score_idx):
        k = self.calls_2d
        self.calls_2d += 1
        return self.listed, list(self.global_s[k * len(x_range):(k + 1) * len(x_range)])

    def score(self, slope, x_max, y_max, score_idx):
        self.lines.append((float(x_max), float(y_max)))
        return np.array(self.eval_stats[len(self.lines) - 1], dtype=np.int64), None


def run(c, scorer, **kw):
    names = ["s%d" % k for k in range(n_of(c))]
    return refine.refineFit(scorer, names, c["mean0"].copy(), c["mean1"].copy(), c["scale"], float(c["max_move"]),
                            float(c["min_move"]), slope=int(c["slope"]), unconstrained=bool(c["unconstrained"]),
                            no_local=bool(c["no_local"]), **kw)


def test_transform_line_and_decision_boundary(golden):
    for r, want in zip(golden["tl_in"], golden["tl_out"]):
        assert np.array_equal(utils.transformLine(r[0], r[1:3], r[3:5]), want)
    for r, want, after in zip(golden["db_in"], golden["db_out"], golden["db_after"]):
        p = r[0:2].copy()
        got = utils.decisionBoundary(p, r[2], adj=r[3])
        assert np.array_equal(np.array(got, dtype=np.float64), want)
        assert np.array_equal(p, after)                  # moved in place when adj != 0 ...
        assert (r[3] != 0.0) == (not np.array_equal(p, r[0:2]))      # ... and only then


LOCAL_CASES = ["slope2_local", "slope0_local", "slope1_local", "slope2_b_local", "unconstrained_local"]
PLAIN_CASES = ["no_local", "min_at_end", "unconstrained_edge"]


@pytest.mark.parametrize("name", LOCAL_CASES + PLAIN_CASES)
def test_local_search_replays_the_reference(golden, name):
    """The recorded counts go through summary_from_stats into scipy's bounded minimiser: it must evaluate the
    reference's positions in the reference's order, return its scores and end at its result.  Measured here: every
    position, score and result equals the golden's exactly (largest relative difference 0), so the bar of the device
    comparison (tests/test_gpu_refine_fit.py) is exact equality."""
    c = case_of(golden, name)
    scorer = Replay(n_of(c), c["global_s"], c["eval_stats"])
    res = run(c, scorer)
    info = refine.last_fit
    assert np.array_equal(info["global_s"], c["global_s"])
    got_s = np.array([e[0] for e in info["evals"]])
    rel = np.max(np.abs(got_s - c["eval_s"]) / np.abs(c["eval_s"])) if got_s.size == c["eval_s"].size and got_s.size else 0.0
    print(name, "evaluations", got_s.size, "largest relative difference of s", rel)
    assert np.array_equal(got_s, c["eval_s"])
    assert np.array_equal(np.array([e[2] for e in info["evals"]]), c["eval_score"])
    assert [e[1] for e in info["evals"]] == c["eval_stats"].tolist()
    if name in LOCAL_CASES:
        assert info["bounds"] == c["bounds"].tolist() and info["local_path"] == "score" and got_s.size > 3
    else:
        assert info["bounds"] is None and c["bounds"].size == 0 and got_s.size == 0
    assert np.array_equal(np.array([float(v) for v in res]), c["result"])


def test_bounds_ends_and_nan_scores():
    c = {"dist": "sweep1d_dist", "mean0": np.array([0.08, 0.06]), "mean1": np.array([0.55, 0.45]),
         "scale": np.array([1.0, 1.0]), "max_move": 0.05, "min_move": 0.04, "slope": 2, "unconstrained": False,
         "no_local": False}
    dx, dy = c["mean1"][0] - c["mean0"][0], c["mean1"][1] - c["mean0"][1]
    s_range = np.linspace(-0.04, 0.05 + (dx**2 + dy**2)**0.5, 40)
    # NaN -> 1: the NaN entries must not win, the minimum is the -0.5 at index 7
    gs = np.full(40, -0.1)
    gs[3] = gs[30] = np.nan
    gs[7] = -0.5
    scorer = Replay(300, gs, [[10, 290, 5, 20]] * 64)
    run(c, scorer)
    info = refine.last_fit
    assert info["global_s"][3] == 1 and info["global_s"][30] == 1
    assert info["bounds"] == [s_range[6], s_range[8]]
    assert all(s_range[6] < e[0] < s_range[8] for e in info["evals"])
    # the minimum at either end: no local step, the offset itself is returned
    for idx in (0, 39):
        gs = np.full(40, -0.1)
        gs[idx] = -0.5
        scorer = Replay(300, gs)
        res = run(c, scorer)
        assert refine.last_fit["bounds"] is None and scorer.lines == [] and res[2] == s_range[idx]
        x, y = utils.decisionBoundary(utils.transformLine(s_range[idx], c["mean0"], c["mean1"]), dy / dx)
        assert (res[0], res[1]) == (x, y)
    # growNetwork's list stops at the last offset with edges: a shorter list, its last entry the minimum, still counts
    # as interior (the reference compares with len(s_range))
    gs = np.full(30, -0.1)
    gs[29] = -0.5
    run(c, Replay(300, gs, [[10, 290, 5, 20]] * 64))
    assert refine.last_fit["bounds"] == [s_range[28], s_range[30]]
    # slopes 0 and 1 return the point on the line itself
    c["slope"], c["no_local"] = 0, True
    res = run(c, Replay(300, gs))
    assert np.array_equal(np.array(res[:2]), utils.transformLine(s_range[29], c["mean0"], c["mean1"]))


def test_grid_indexing_of_the_unconstrained_search():
    c = {"dist": "sweep2d_dist", "mean0": np.array([0.08, 0.06]), "mean1": np.array([0.55, 0.45]),
         "scale": np.array([1.0, 1.0]), "max_move": 0.05, "min_move": 0.04, "slope": 2, "unconstrained": True,
         "no_local": True}
    m0, m1 = c["mean0"].copy(), c["mean1"].copy()
    g = (m1[1] - m0[1]) / (m1[0] - m0[0])
    xs, ys = utils.decisionBoundary(m0, g, adj=-0.04)
    xe, ye = utils.decisionBoundary(m1, g, adj=0.05)
    x_max, y_max = np.linspace(xs, xe, 20, dtype=np.float32), np.linspace(ys, ye, 20, dtype=np.float32)
    for xi, yi in ((3, 11), (0, 5), (19, 19), (7, 0)):
        gs = np.zeros(400)
        gs[yi * 20 + xi] = -0.7          # row y, column x: the lists of the 20 y values back to back
        scorer = Replay(200, gs)
        res = run(c, scorer)
        assert scorer.calls_2d == 20
        assert res[0] == x_max[xi] and res[1] == y_max[yi] and res[2] == -0.7
    # a y whose boundary lists every row scores zeros: nothing recorded wins against them here
    scorer = Replay(200, np.full(400, 0.3), listed=200 * 199 // 2)
    res = run(c, scorer)
    assert np.array_equal(refine.last_fit["global_s"], np.zeros(400)) and res[2] == 0
    # interior minimum with a local step: the reference's parameterisation
    c["no_local"] = False
    gs = np.zeros(400)
    gs[11 * 20 + 3] = -0.7
    scorer = Replay(200, gs, [[10, 190, 5, 20]] * 64)
    run(c, scorer)
    delta = x_max[1] - x_max[0]
    assert refine.last_fit["bounds"] == [float(-delta), float(delta)]
    gradient = x_max[3] / y_max[11]
    mean1 = (x_max[3] + delta, delta * gradient)
    s0 = refine.last_fit["evals"][0][0]
    want = utils.decisionBoundary(utils.transformLine(s0, m0, mean1), gradient)      # m0: moved by adj, as upstream
    assert scorer.lines[0] == (float(want[0]), float(want[1]))


def test_error_texts(golden):
    for name in ("below_zero", "all_points"):
        c = case_of(golden, name)
        scorer = Replay(n_of(c), np.full(40, -0.1), listed=n_of(c) * (n_of(c) - 1) // 2 if name == "all_points" else 0)
        with pytest.raises(RuntimeError) as e:
            run(c, scorer)
        assert str(e.value) == str(c["error"])
    c = case_of(golden, "below_zero")
    c["unconstrained"] = True
    with pytest.raises(RuntimeError, match="^Boundary range below zero$"):
        run(c, Replay(300, np.zeros(400)))
    c = case_of(golden, "slope0_local")
    c["unconstrained"] = True
    with pytest.raises(RuntimeError, match="^Unconstrained optimization and indiv-refine incompatible$"):
        run(c, Replay(300, np.zeros(400)))
    # a local search that ends below zero (only reachable with a line that leaves the positive quadrant)
    c = case_of(golden, "slope2_local")
    c["mean0"], c["mean1"], c["min_move"], c["max_move"] = np.array([0.3, 0.02]), np.array([0.5, -0.4]), 0.0, 0.0
    gs = np.full(40, -0.1)
    gs[38] = -0.5
    with pytest.raises(RuntimeError, match="^Boundary range below zero$"):
        run(c, Replay(300, gs, [[10, 290, 5, 20]] * 64))
    # sample_size is refused before anything else happens
    for call in (lambda: run(case_of(golden, "slope2_local"), None, sample_size=10),
                 lambda: refine.newNetwork(0.1, ["a"], None, None, None, 1.0, sample_size=10),
                 lambda: refine.newNetwork2D(0, ["a"], None, None, None, sample_size=10),
                 lambda: models.RefineBoundary().fit(None, None, None, 0.1, 0.1, sample_size=10)):
        with pytest.raises(NotImplementedError, match="sample_size"):
            call()


def test_new_network_is_one_score(golden):
    c = case_of(golden, "slope2_local")
    k = 2
    scorer = Replay(300, [], [c["eval_stats"][k]])
    g = (c["mean1"][1] - c["mean0"][1]) / (c["mean1"][0] - c["mean0"][0])
    got = refine.newNetwork(c["eval_s"][k], ["s"] * 300, scorer, c["mean0"], c["mean1"], g)
    assert got == c["eval_score"][k]
    assert scorer.lines == [tuple(float(v) for v in refine.boundary_of_s(c["eval_s"][k], c["mean0"], c["mean1"], g))]
    assert refine.boundary_of_s(0.1, c["mean0"], c["mean1"], g, 0)[1] == 0
    assert refine.boundary_of_s(0.1, c["mean0"], c["mean1"], g, 1)[0] == 0


def test_read_manual_start(tmp_path):
    p = tmp_path / "start.txt"
    p.write_text("start 0.1,0.2\nend 0.5,0.6\n")
    m0, m1, scaled = refine.readManualStart(str(p))
    assert np.array_equal(m0, [0.1, 0.2]) and np.array_equal(m1, [0.5, 0.6]) and scaled is True
    p.write_text("end 0.5,0.6\nscaled false\nstart 0.1,0.2\n")
    assert refine.readManualStart(str(p))[2] is False
    p.write_text("begin 0.1,0.2\n")
    with pytest.raises(RuntimeError, match="^Incorrectly formatted manual start file$"):
        refine.readManualStart(str(p))
    for text, why in (("start 0.1,0.2\n", "Must set both start and end"),
                      ("start 0.1,0.2,0.3\nend 0.5,0.6\n", "Wrong size for values"),
                      ("start 0.1,1.2\nend 0.5,0.6\n", "Value out of range (between 0 and 1)")):
        p.write_text(text)
        with pytest.raises(SystemExit) as e:
            refine.readManualStart(str(p))
        assert e.value.code == 1


def test_manual_start_messages(tmp_path, capsys):
    p = tmp_path / "start.txt"
    p.write_text("start 0.1,0.2\n")
    with pytest.raises(SystemExit):
        refine.readManualStart(str(p))
    err = capsys.readouterr().err
    assert err == "Could not read manual start file %s\nMust set both start and end\n" % p


def test_npz_round_trip_and_reference_keys(tmp_path):
    b = models.RefineBoundary(scale=(0.05, 0.25), optimal_x=0.31, optimal_y=0.37, core_boundary=0.2,
                              accessory_boundary=0.16)
    b.indiv_fitted = True
    path = b.save(tmp_path / "db")
    assert os.path.basename(path) == "db_fit.npz"
    with np.load(path) as z:
        assert sorted(z.files) == ["core_acc_intercepts", "indiv_fitted", "intercept", "scale"]
        assert np.array_equal(z["intercept"], [0.31, 0.37]) and np.array_equal(z["core_acc_intercepts"], [0.2, 0.16])
    c = models.RefineBoundary.from_npz(path)
    assert (c.optimal_x, c.optimal_y, c.core_boundary, c.accessory_boundary) == (0.31, 0.37, 0.2, 0.16)
    assert c.indiv_fitted is True and c.fitted and not c.threshold and np.array_equal(c.scale, b.scale)
    assert c.scale.dtype == np.float32 and c.slope == 2
    with pytest.raises(RuntimeError, match="unfitted"):
        models.RefineBoundary().save(tmp_path / "none")
    # a file as PopPUNK writes it: float64 scale; older ones have no indiv_fitted
    ref = tmp_path / "ref_fit.npz"
    np.savez(ref, intercept=np.array([0.4, 0.5]), core_acc_intercepts=np.array([0.4, 0.5]),
             scale=np.array([0.03, 0.3], dtype=np.float64))
    c = models.RefineBoundary.from_npz(str(ref))
    assert c.indiv_fitted is False and not c.threshold and c.optimal_y == 0.5
    # apply_threshold's model: NaN in both second entries marks a threshold model
    np.savez(ref, intercept=np.array([0.02, np.nan]), core_acc_intercepts=np.array([0.02, np.nan]),
             scale=np.array([1, 1], dtype=np.float32), indiv_fitted=False)
    c = models.RefineBoundary.from_npz(str(ref))
    assert c.threshold and c.core_boundary == 0.02
    with pytest.raises(ValueError, match="not a refine fit"):
        models.RefineBoundary.from_npz({"weights": np.ones(2)})


def test_golden_covers_the_cases(golden):
    assert sorted(golden["cases"].tolist()) == sorted(LOCAL_CASES + PLAIN_CASES + ["below_zero", "all_points"])
    with np.load(SWEEP) as z:
        assert z["sweep1d_dist"].shape == (300 * 299 // 2, 2) and z["sweep2d_dist"].shape == (200 * 199 // 2, 2)
    for name in LOCAL_CASES:
        c = case_of(golden, name)
        assert c["eval_s"].size >= 5 and c["bounds"].size == 2 and c["eval_stats"].shape == (c["eval_s"].size, 4)
        assert np.all((c["eval_s"] > c["bounds"][0]) & (c["eval_s"] < c["bounds"][1]))
