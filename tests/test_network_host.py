"""CPU tests of the network-score mirror (poppunk_amd/refine.py): the per-offset counts -> networkSummary metrics
and growNetwork's score list, against tests/golden/network_sweep.npz (the reference's own growNetwork and
networkSummary, make_golden_network.py); what is not mirrored raises before any device is touched."""
import os

import numpy as np
import pytest

from poppunk_amd import refine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "network_sweep.npz")


def golden():
    z = np.load(GOLDEN)
    return z, [str(c) for c in z["cases"]]


def assert_scores(got, want):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)


def test_golden_covers_the_quirk():
    z, cases = golden()
    assert set(cases) == {"sweep1d", "sweep2d", "holes", "late"}
    # absent offsets inside the list, a first index above 0, NaN transitivity at the start of a sweep
    assert z["holes_present"].size < int(z["holes_n_off"])
    assert int(z["late_present"][0]) > 0
    assert np.isnan(z["sweep1d_scores"]).any()


@pytest.mark.parametrize("case", ["sweep1d", "sweep2d", "holes", "late"])
def test_metrics_from_counts_match_network_summary(case):
    z, _ = golden()
    n = int(z[case + "_n"])
    stats = z[case + "_stats"]
    for t, want in zip(z[case + "_present"], z[case + "_metrics"]):
        metrics, scores = refine.summary_from_stats(stats[t], n)
        assert metrics[0] == want[0] and metrics[1] == want[1]          # components, density: exact
        assert (np.isnan(metrics[2]) and np.isnan(want[2])) or metrics[2] == want[2]
        assert metrics[3] == 0 and metrics[4] == 0
        assert scores[0] == scores[1] == scores[2] or np.isnan(scores[0])


@pytest.mark.parametrize("case", ["sweep1d", "sweep2d", "holes", "late"])
def test_score_list_from_counts_matches_grow_network(case):
    z, _ = golden()
    got = refine.grow_scores(z[case + "_stats"], int(z[case + "_n"]))
    assert len(got) == int(z[case + "_idx"].max()) + 1
    assert_scores(got, z[case + "_scores"])


def test_grow_scores_quirk_by_hand():
    n = 4
    # offsets 0: no edges; 1: (0,1); 2: nothing new; 3: (1,2), (0,2) -> a triangle
    stats = np.array([[0, 4, 0, 0], [1, 3, 0, 0], [1, 3, 0, 0], [3, 2, 1, 3]])
    got = refine.grow_scores(stats, n)
    base3 = -(3 * 1 / 3) * (1 - 3 / 6)
    assert len(got) == 4
    assert np.isnan(got[0]) and np.isnan(got[1])       # idx 1 (W = 0) appended idx - (-1) = 2 times
    assert got[2] == base3 and got[3] == base3         # idx 3 appended 3 - 1 = 2 times
    with pytest.raises(ValueError):
        refine.grow_scores(np.array([[0, 4, 0, 0]]), n)


@pytest.mark.parametrize("kw", [{"score_idx": 1}, {"score_idx": 2}, {"sample_size": 10},
                                {"write_clusters": "out/prefix"}])
def test_unmirrored_options_raise_before_the_device(kw, monkeypatch):
    from poppunk_amd import _lib

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    with pytest.raises(NotImplementedError):
        refine.growNetwork(["a", "b", "c"], [0], [1], [0], [0.0], **kw)


def test_empty_input_is_a_value_error(monkeypatch):
    from poppunk_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    with pytest.raises(ValueError):
        refine.growNetwork(["a", "b"], [], [], [], [])
    # use_gpu is accepted (and ignored) like the other reference arguments
    with pytest.raises(ValueError):
        refine.growNetwork(["a", "b"], [], [], [], [], thread_idx=3, betweenness_sample=50, use_gpu=True)
