"""GPU tests of the silhouette (ppk_silhouette*, engine.silhouette_dev, poppunk_amd.scores): a, b and
s of every sample against the numpy restatement of the rule (tests/silhouette_model.py) BIT FOR BIT, and against
sklearn's recorded arrays (tests/golden/silhouette.npz) within the derived bound; every routing option against the
default routing bit for bit; the first-offender errors by message."""
import ctypes as C
import os

import numpy as np
import pytest

import silhouette_model as model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, scores  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
SIZES = [3, 5, 64, 65, 130, 257]      # the smallest legal n; under / at / over a tile edge; two tiles and a remainder


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def matrix(n, seed=0):
    """float32 [n(n-1)/2, 2] in [0, 1]: ordinary magnitudes, a tenth of the rows below 2^-17, some exact zeros."""
    rng = np.random.default_rng(1000 * n + seed)
    rows = n * (n - 1) // 2
    x = rng.random((rows, 2)) * np.array([0.05, 0.3])
    small = rng.random(rows) < 0.1
    x[small] = 2.0 ** rng.uniform(-36, -18, (int(small.sum()), 2))
    x[rng.random(rows) < 0.02] = 0.0
    return x.astype(np.float32)


def labelings(n, seed=0):
    rng = np.random.default_rng(77 * n + seed)
    two = rng.integers(1, 3, n)
    two[0], two[1] = 1, 2
    pair = np.arange(1, n + 1)
    pair[n // 2] = pair[0]                                  # n - 1 labels: one pair, the rest singletons
    mix = np.where(rng.random(n) < 0.6, 2, rng.integers(3, min(n, max(4, n // 4)) + 1, n))
    mix[-max(1, n // 16):] = n - np.arange(max(1, n // 16))  # singletons at the end, one large cluster, a few small
    values = np.array([1, 5, n] if n >= 5 else [1, n])
    gaps = values[rng.integers(0, len(values), n)]
    gaps[0], gaps[-1] = 1, n
    return {k: v.astype(np.int32) for k, v in (("two", two), ("pair", pair), ("mix", mix), ("gaps", gaps))}


def run(x, levels, metric=2, shift=None):
    s, n_labels, valid, a, b = engine.silhouette_dev(dev(x), dev(np.atleast_2d(levels).astype(np.int32)), metric=metric,
                                                     shift=shift, want_ab=True)
    return a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy(), n_labels.cpu().numpy(), valid.cpu().numpy()


def assert_same(got, want, what=""):
    for g, w, name in zip(got[:3], want[:3], "abs"):
        assert model.same_bits(g, w), (what, name, int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))))
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), (what, got[3], got[4])


@pytest.mark.parametrize("metric", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_labelings_against_the_model(n, metric):
    x, lab = matrix(n), labelings(n)
    three = np.stack([lab["two"], lab["pair"], lab["mix"]])
    assert_same(run(x, three, metric), model.silhouette(x, three, metric), "3 levels")
    assert_same(run(x, lab["gaps"], metric), model.silhouette(x, lab["gaps"], metric), "1 level")


def test_invalid_levels_are_nan_and_leave_the_others_alone():
    n = 65
    x, lab = matrix(n), labelings(n)
    levels = np.stack([lab["two"], np.full(n, 7, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)])
    a, b, s, n_labels, valid = run(x, levels)
    assert valid.tolist() == [1, 0, 0] and n_labels.tolist() == [2, 1, n]
    for arr in (a, b, s):
        assert np.all(np.isnan(arr[1:])) and not np.any(np.isnan(arr[0]))
    alone = run(x, lab["two"])
    for arr, one in zip((a, b, s), alone[:3]):
        assert np.array_equal(arr[0], one[0])
    assert_same((a, b, s, n_labels, valid), model.silhouette(x, levels, 2))


@pytest.mark.parametrize("metric", [0, 2, 3])
def test_zero_and_constant_matrices(metric):
    n = 65
    lab = labelings(n)
    levels = np.stack([lab["two"], lab["mix"]])
    a, b, s, _, valid = run(np.zeros((n * (n - 1) // 2, 2), dtype=np.float32), levels, metric)
    assert valid.tolist() == [1, 1]
    assert np.all(a == 0) and np.all(b == 0) and np.all(s == 0)
    a, b, s, _, _ = run(np.full((n * (n - 1) // 2, 2), 0.25, dtype=np.float32), levels, metric if metric != 3 else 2)
    assert np.array_equal(a, b) and np.all(s == 0)
    single = np.bincount(lab["mix"], minlength=n + 1)[lab["mix"]] == 1
    assert single.any() and np.all(a[1][single] == 0) and np.all(a[1][~single] > 0)


def test_golden_cases_against_the_model_and_sklearn():
    z = np.load(os.path.join(HERE, "golden", "silhouette.npz"))
    for k in range(int(z["n_cases"])):
        x, labels = z["case%d_x" % k], z["case%d_labels" % k]
        n = len(labels)
        for metric in range(4):
            got = run(x, labels, metric)
            assert_same(got, model.silhouette(x, labels, metric), "case %d metric %d" % (k, metric))
            sk, a_ref, b_ref = (z["case%d_%s%d" % (k, what, metric)] for what in ("sk", "a", "b"))
            eps, allowed = model.bound(x, metric, n, a_ref, b_ref)
            worst = np.abs(got[2][0] - sk)
            print("case %d metric %d: max |s - sklearn| %.3g, eps %.3g" % (k, metric, worst.max(), eps))
            assert np.abs(got[0][0] - a_ref).max() <= eps and np.abs(got[1][0] - b_ref).max() <= eps
            assert np.all(worst <= allowed), (k, metric, float(worst.max()))


@pytest.fixture(scope="module")
def routed():
    """The default routing's results, computed once: n = 130 with three levels (two clusters, 129 labels, the mix),
    n = 257 with 40 labels, n = 520 (where a 1 MB cap cuts the samples into two bands)."""
    out = {}
    x, lab = matrix(130), labelings(130)
    out[130] = (x, np.stack([lab["two"], lab["pair"], lab["mix"]]))
    rng = np.random.default_rng(5)
    forty = (rng.integers(0, 40, 257) * 6 + 1).astype(np.int32)      # 40 labels spread over [1, 235]
    forty[:40] = np.arange(40) * 6 + 1
    out[257] = (matrix(257), np.stack([forty, labelings(257)["mix"]]))
    out[520] = (matrix(520), np.stack([labelings(520)["two"], labelings(520)["mix"]]))
    return {n: (x, lv, run(x, lv)) for n, (x, lv) in out.items()}


@pytest.mark.parametrize("option,value,n", [("silhouette_band", 1, 130), ("silhouette_band", 7, 130),
                                            ("silhouette_band", 64, 130), ("silhouette_band", 65, 130),
                                            ("silhouette_window", 8, 130), ("silhouette_window", 8, 257),
                                            ("silhouette_scratch_mb", 1, 520)])
def test_every_routing_gives_the_bits_of_the_default(routed, ppk_option, option, value, n):
    x, levels, want = routed[n]
    if n == 130:
        assert want[3][1] == 129
    ppk_option(option, value)
    assert_same(run(x, levels), want, "%s = %d" % (option, value))


def test_default_routing_of_the_routed_shapes_against_the_model(routed):
    for n in (130, 257):
        x, levels, want = routed[n]
        assert_same(want, model.silhouette(x, levels, 2), "n = %d" % n)


def test_repeated_calls_and_permuted_levels_give_identical_bits(routed):
    x, levels, want = routed[130]
    assert_same(run(x, levels), want, "second call")
    perm = [2, 0, 1]
    got = run(x.copy(), levels[perm])
    assert_same(got, tuple(w[perm] for w in want), "permuted levels")


def test_first_offender_errors_name_the_row_or_the_level_and_vertex():
    n = 65
    x, lab = matrix(n), labelings(n)
    levels = np.stack([lab["two"], lab["mix"]])
    for row, col, value, text in ((1234, 0, np.nan, "nan"), (77, 1, 1.5, "1.500000"), (2000, 0, -0.25, "-0.250000"),
                                  (5, 1, np.inf, "inf")):
        bad = x.copy()
        bad[row, col] = value
        bad[row + 40, 1 - col] = 2.0                        # a later offender: the first one is named
        for metric in (0, 1, 2):                            # either column, whatever the metric
            with pytest.raises(RuntimeError) as e:
                run(bad, levels, metric)
            assert "ppk_silhouette: row %d, column %d: value %s is not a finite number in [0, 1]" % (row, col, text) \
                in str(e.value)
    for level, vertex, value in ((1, 3, 0), (0, 64, n + 1), (1, 0, -4)):
        bad = levels.copy()
        bad[level, vertex] = value
        with pytest.raises(RuntimeError) as e:
            run(x, bad)
        assert "ppk_silhouette: level %d, vertex %d: label %d outside [1, %d]" % (level, vertex, value, n) in str(e.value)
    # the call after a refused one is unaffected
    assert_same(run(x, levels), model.silhouette(x, levels, 2))


def test_host_form_equals_the_device_form(routed):
    x, levels, want = routed[130]
    n_levels, n = levels.shape
    a, b, s = (np.empty((n_levels, n), dtype=np.float64) for _ in range(3))
    n_labels, valid = np.empty(n_levels, dtype=np.int32), np.empty(n_levels, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    _lib.check(_lib.lib().ppk_silhouette(x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], 2, lv.ctypes.data_as(ip),
                                         n_levels, engine.silhouette_shift(n), 0, a.ctypes.data_as(dp),
                                         b.ctypes.data_as(dp), s.ctypes.data_as(dp), n_labels.ctypes.data_as(ip),
                                         valid.ctypes.data_as(ip)), "ppk_silhouette")
    assert_same((a, b, s, n_labels, valid), want, "host form")
    # ... and without a, b, as poppunk_amd.scores calls it
    s2, n_labels2, valid2 = scores._device_silhouette(x, lv, 2)
    assert model.same_bits(s2, want[2]) and np.array_equal(n_labels2, want[3]) and np.array_equal(valid2, want[4])


def test_scores_on_numpy_and_resident_matrices():
    n = 130
    x, lab = matrix(n), labelings(n)
    names = ["c%d" % c for c in lab["mix"]]
    for name, code in scores.METRICS.items():
        want = model.silhouette(x, scores.factorise(names)[0], code)[2][0]
        assert scores.silhouette_score(x, names, metric=name) == float(np.mean(want))
        assert np.array_equal(scores.silhouette_samples(dev(x), names, metric=name), want)
    with pytest.raises(ValueError, match="Number of labels is 1. Valid values are 2 to n_samples - 1"):
        scores.silhouette_score(x, ["a"] * n)
    # a smaller shift is the same rule at another resolution
    assert_same(run(x, lab["mix"], 2, shift=20), model.silhouette(x, lab["mix"], 2, shift=20), "shift 20")


def test_row_indices_past_2_to_the_31():
    """n = 46 342: 1 073 767 311 rows, so the float index 2k of a row passes 2^31 (and 2^32 bytes many times over).
    Four samples, the first and last rows of the matrix among theirs, against the same integer sums taken with torch
    through int64 row indices."""
    n = 46342
    n_rows = n * (n - 1) // 2
    assert 2 * n_rows > 1 << 31
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    x = torch.rand((n_rows, 2), device=DEV, dtype=torch.float32, generator=gen) * 0.125
    labels = (torch.arange(n, device=DEV) % 7 + 1).to(torch.int32)
    shift = engine.silhouette_shift(n)
    s, n_labels, valid, a, b = engine.silhouette_dev(x, labels[None, :].contiguous(), metric=0, want_ab=True)
    assert n_labels.tolist() == [7] and valid.tolist() == [1]
    cnt = torch.bincount(labels.long(), minlength=8).cpu().numpy()
    for i in (0, 1, 40001, n - 1):
        j = torch.cat([torch.arange(0, i, device=DEV), torch.arange(i + 1, n, device=DEV)])
        lo, hi = torch.clamp(j, max=i), torch.clamp(j, min=i)
        k = lo * n - (lo * (lo + 1)) // 2 + (hi - lo - 1)
        q = torch.round(x[k, 0].double() * 2.0 ** shift).long()
        T = torch.zeros(8, dtype=torch.int64, device=DEV).index_add_(0, labels[j].long(), q).cpu().numpy()
        ci = int(labels[i])
        others = [c for c in range(1, 8) if c != ci]
        want_a = (np.float64(T[ci]) * 2.0 ** -shift) / np.float64(cnt[ci] - 1)
        want_b = np.min((T[others].astype(np.float64) * 2.0 ** -shift) / cnt[others].astype(np.float64))
        assert float(a[0, i]) == want_a and float(b[0, i]) == want_b, i
        assert float(s[0, i]) == (want_b - want_a) / max(want_a, want_b), i


def test_silhouette_of_levels_on_a_cluster_sweep():
    """Three graphs on 64 samples in four planted groups: no edges (64 singletons: invalid), the within-group pairs
    (four clusters), every pair (one cluster: invalid).  NaN exactly at the invalid levels."""
    n = 64
    groups = np.arange(n) % 4
    i, j = np.triu_indices(n, 1)
    same = groups[i] == groups[j]
    rng = np.random.default_rng(3)
    x = np.where(same[:, None], rng.uniform(0.001, 0.01, (len(i), 2)), rng.uniform(0.02, 0.06, (len(i), 2)))
    x = x.astype(np.float32)
    off = np.where(same, 1, 2).astype(np.int64)
    clusters, counts = engine.cluster_sweep_dev(dev(i.astype(np.int64)), dev(j.astype(np.int64)), dev(off), n, 3)
    assert counts.cpu().numpy().tolist() == [n, 4, 1]
    means = scores.silhouette_of_levels(dev(x), clusters)
    _, _, s, _, valid = model.silhouette(x, clusters.cpu().numpy(), 2)
    assert valid.tolist() == [0, 1, 0]
    assert np.isnan(means).tolist() == [True, False, True]
    assert means[1] == np.mean(s[1]) and means[1] > 0.5
