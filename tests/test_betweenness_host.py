"""CPU tests of networkSummary with betweenness (poppunk_amd/refine.py, poppunk_amd/network.py): the metrics and
growNetwork's score_idx 1 / 2 lists from the counts plus the betweenness means, print_network_summary's text,
against tests/golden/network_betweenness.npz (the reference's own networkSummary, print_network_summary and
growNetwork, make_golden_betweenness.py); subsampling raises before any device is touched."""
import os

import numpy as np
import pytest

from poppunk_amd import network, refine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "network_betweenness.npz")
SWEEP = os.path.join(HERE, "golden", "network_sweep.npz")


def assert_scores(got, want):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)


def test_golden_has_betweenness_to_test():
    g = np.load(GOLDEN)
    for case in ("sweep1d", "sweep2d"):
        assert (g[case + "_bt"] > 0).any()
        assert not np.array_equal(g[case + "_scores1"], g[case + "_scores2"])
    assert int(g["mix_scored"]) > 40 and g["mix_metrics"][3] > 0
    assert int(g["tiny_scored"]) == 0 and np.isnan(g["tiny_metrics"][2])


@pytest.mark.parametrize("case", ["sweep1d", "sweep2d"])
@pytest.mark.parametrize("score_idx", [1, 2])
def test_score_lists_from_counts_and_bt_match_grow_network(case, score_idx):
    g, z = np.load(GOLDEN), np.load(SWEEP)
    got = refine.grow_scores(z[case + "_stats"], int(z[case + "_n"]), score_idx, bt=g[case + "_bt"])
    assert_scores(got, g["%s_scores%d" % (case, score_idx)])
    # score_idx 0 ignores bt: today's list
    assert_scores(refine.grow_scores(z[case + "_stats"], int(z[case + "_n"]), 0, bt=g[case + "_bt"]),
                  z[case + "_scores"])


@pytest.mark.parametrize("case", ["sweep1d", "sweep2d"])
def test_metrics_with_bt_match_network_summary(case):
    g, z = np.load(GOLDEN), np.load(SWEEP)
    n = int(z[case + "_n"])
    for t, want in zip(g[case + "_present"], g[case + "_metrics"]):
        metrics, scores = refine.summary_from_stats(z[case + "_stats"][t], n, g[case + "_bt"][t])
        assert metrics[0] == want[0] and metrics[1] == want[1]
        assert (np.isnan(metrics[2]) and np.isnan(want[2])) or metrics[2] == want[2]
        assert metrics[3] == want[3] and metrics[4] == want[4]
        base = scores[0]
        assert (np.isnan(base) and np.isnan(scores[1])) or scores[1] == base * (1 - want[3])
        assert (np.isnan(base) and np.isnan(scores[2])) or scores[2] == base * (1 - want[4])


def test_score_mapping_by_hand():
    stats = np.array([[0, 5, 0, 0], [3, 2, 0, 3], [4, 1, 1, 5]])
    bt = np.array([[0.0, 0.0], [0.5, 0.25], [0.4, 0.2]])
    metrics, scores = refine.summary_from_stats(stats[2], 5, bt[2])
    base = (3 * 1 / 5) * (1 - 4 / 10)
    assert metrics == [1, 0.4, 0.6, 0.4, 0.2]
    assert scores == [base, base * (1 - 0.4), base * (1 - 0.2)]
    got = refine.grow_scores(stats, 5, 2, bt=bt)
    assert len(got) == 3 and got[0] == got[1] == 0 and got[2] == -base * (1 - 0.2)
    with pytest.raises(ValueError):
        refine.grow_scores(stats, 5, 1)                 # betweenness scores need bt
    with pytest.raises(ValueError):
        refine.grow_scores(stats, 5, 3, bt=bt)
    with pytest.raises(ValueError):
        refine.grow_scores(stats, 5, 1, bt=bt[:2])


@pytest.mark.parametrize("case", ["mix", "tiny"])
def test_print_network_summary_text(case, capsys, monkeypatch):
    g = np.load(GOLDEN)
    n = int(g[case + "_n"])

    def summary_from_golden(i, j, idx, n_, n_off=None, values_at=None, device=0):
        assert n_ == n and np.array_equal(np.stack([i, j], axis=1), g[case + "_edges"])
        return g[case + "_stats"][None], g[case + "_metrics"][None, 3:5], None, None
    monkeypatch.setattr(refine, "network_summary", summary_from_golden)
    network.print_network_summary((g[case + "_edges"], n))
    assert capsys.readouterr().err == str(g[case + "_text"])
    metrics, scores = network.networkSummary((g[case + "_edges"], n), betweenness_sample=10, use_gpu=True)
    assert metrics[0] == g[case + "_metrics"][0]
    assert_scores(scores, g[case + "_scores"])


def test_subsample_raises_before_the_device(monkeypatch):
    from poppunk_amd import _lib

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    e = np.array([[0, 1], [1, 2]], dtype=np.int64)
    with pytest.raises(NotImplementedError):
        network.networkSummary((e, 4), subsample=2)
    with pytest.raises(NotImplementedError):
        network.print_network_summary((e, 4), sample_size=2)
