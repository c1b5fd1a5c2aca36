"""The embedding's calibration and loop at every branch and edge shape (ppk_embed.hip): the weight
kernels' grid strides and unreachable rows, the loop's options, schedule, worker counts, seeds, zero weights, exact
prefix hits, clips, skips and contention, each bit for bit against the restatement (tests/test_embed_host.py), whose
`stats` show that a case does what it is named for; every argument error by its message, each followed by a good call.
Every loop case runs at most 400 iterations."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine  # noqa: E402
from test_embed_host import (HAND_MADE, HARD_SHAPES, calibrate, embed, generated_lists, hand_made_P,  # noqa: E402
                             init_positions, knn_lists, neighbour_ring, row_conditions, run_stats, schedule,
                             star_lists, unreachable_case, weights)

DEV = "cuda:0"
RTOL = 1e-12           # P against the restatement, on well-conditioned rows


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def cuda(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device=DEV)


def device_weights(i, j, d, n, perp=20.0):
    """P of the device; c == weights(P) bit for bit is asserted on every call"""
    P, c = engine.embed_weights_dev(cuda(i, np.int64), cuda(j, np.int64), cuda(d, np.float32), n, perp,
                                    weights=True)
    P = P.cpu().numpy()
    assert np.array_equal(c.cpu().numpy().view(np.uint64), weights(P))
    return P


def device_embed(i, j, P, n, seed, max_iter, **kw):
    return engine.embed_dev(cuda(i, np.int64), cuda(j, np.int64), cuda(P, np.float64), n, seed, max_iter=max_iter,
                            **kw).cpu().numpy()


def both(i, j, P, n, seed, max_iter, **kw):
    """Y of the device, equal bit for bit to the restatement's; and the restatement's stats"""
    Y = device_embed(i, j, P, n, seed, max_iter, **kw)
    want, st = run_stats(P, i, j, n, seed=seed, max_iter=max_iter, **kw)
    assert Y.shape == (n, 2) and np.all(np.isfinite(Y))
    assert np.array_equal(bits(Y), bits(want)), (np.abs(Y - want).max(), st)
    return Y, st


_planted = {}


def planted_P(n, k, perp=None):
    """(i, j, dist, device P) of planted lists, computed once per shape; perplexity 5 where k allows it"""
    perp = perp or (5.0 if k >= 8 else 20.0)
    if (n, k, perp) not in _planted:
        i, j, d = generated_lists("planted", n, k)
        _planted[n, k, perp] = (i, j, d, device_weights(i, j, d, n, perp))
    return _planted[n, k, perp]


def rel_diff(P, want, floor=1e-290):
    big = want > floor
    return float(np.max(np.abs(P[big] - want[big]) / want[big])) if big.any() else 0.0


# ---- calibration -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,perp", [(2, 1, 20.0), (3, 2, 20.0), (130, 129, 20.0), (257, 16, 5.0), (1025, 7, 3.0),
                                      (1100, 1023, 20.0)])
def test_weights_shapes(n, k, perp):
    i, j, d = generated_lists("planted", n, k)
    P = device_weights(i, j, d, n, perp)
    want = calibrate(d, n, k, perp)
    print("n = %d, k = %d: largest relative difference %.3g" % (n, k, rel_diff(P, want)))
    assert np.allclose(P, want, rtol=RTOL, atol=0)
    assert np.allclose(P.reshape(n, k).sum(axis=1), 1.0 / n, rtol=RTOL, atol=0)


@pytest.fixture(scope="module")
def strided():
    """uniform rows at (3000, 40), past the 65 536 entries of one pass of the sum of squares, and at (20 000, 60),
    past the 2^20 of check and quantise: (i, j, dist, restatement's P)"""
    out = {}
    for n, k in ((3000, 40), (20000, 60)):
        i, j, d = generated_lists("uniform", n, k)
        out[n] = (i, j, d, k, calibrate(d, n, k, 20.0))
    return out


@pytest.mark.parametrize("n", [3000, 20000])
def test_weights_grid_strides(strided, n):
    i, j, d, k, want = strided[n]
    assert n * k > (65536 if n == 3000 else 1 << 20)
    P = device_weights(i, j, d, n)
    print("n = %d, k = %d: largest relative difference %.3g" % (n, k, rel_diff(P, want)))
    assert np.allclose(P, want, rtol=RTOL, atol=0)
    # all distances times 2^10: the rms takes the scale, so P keeps its bits wherever the restatement's does
    big = d * np.float32(1024.0)
    Pb = device_weights(i, j, big, n)
    if np.array_equal(bits(calibrate(big, n, k, 20.0)), bits(want)):
        assert np.array_equal(bits(Pb), bits(P))
    else:
        for got in (P, Pb):
            worst = row_conditions(got, d, n, k, 20.0)
            assert max(worst.values()) < 1, worst
    # the loop's check and quantise stride over the same entries: one iteration, bit for bit
    both(i, j, P, n, seed=2, max_iter=n)


def test_weights_name_a_bad_entry_past_a_stride(strided):
    i, j, d, k, want = strided[20000]
    m = 20000 * k
    for e in (m - 1, (1 << 20) + 3):
        dd = d.copy()
        dd[e] = np.nan
        with pytest.raises(RuntimeError) as ex:
            device_weights(i, j, dd, 20000)
        assert "entry %d " % e in str(ex.value) and "NaN" in str(ex.value), str(ex.value)
    Pn = want.copy()
    Pn[(1 << 20) + 3] = -0.25
    Pn[m - 1] = np.nan
    with pytest.raises(RuntimeError) as ex:
        device_embed(i, j, Pn, 20000, seed=1, max_iter=20000)
    assert "entry %d " % ((1 << 20) + 3) in str(ex.value) and "negative" in str(ex.value), str(ex.value)
    assert np.allclose(device_weights(i, j, d, 20000), want, rtol=RTOL, atol=0)


@pytest.mark.parametrize("n,k,perp", HARD_SHAPES)
@pytest.mark.parametrize("kind", ["wide", "one_near"])
def test_hard_rows_meet_the_row_conditions(kind, n, k, perp):
    """Rows whose beta is ill-conditioned (H(beta) nearly flat): the restatement itself is 2e-10 from the converged
    solution there, so the device is held to the conditions that do not depend on the libm, not to 1e-12."""
    i, j, d = generated_lists(kind, n, k)
    P = device_weights(i, j, d, n, perp)
    worst = row_conditions(P, d, n, k, perp)
    print("%s n = %d, k = %d, perplexity %g: ratios %s; against the restatement %.3g relative"
          % (kind, n, k, perp, {key: round(v, 3) for key, v in worst.items()},
             rel_diff(P, calibrate(d, n, k, perp))))
    assert np.all(np.isfinite(P)) and np.all(P >= 0)
    assert max(worst.values()) < 1, worst


UNREACHABLE = ["duplicates", "small_n", "equal", "all_zero", "perp_is_k", "k1_low", "k1_high", "perp_one",
               "denormal", "huge"]


@pytest.mark.parametrize("case", UNREACHABLE)
def test_defined_when_unreachable_on_the_device(case):
    if case in ("duplicates", "small_n", "equal"):
        D, n, k, perp = unreachable_case(case)
        i, j, d = knn_lists(D, k)
    elif case == "all_zero":
        n, k, perp = 40, 7, 3.0
        i, j = neighbour_ring(n, k)
        d = np.zeros(n * k, dtype=np.float32)
    elif case in ("k1_low", "k1_high"):
        n, k, perp = 130, 1, 0.5 if case == "k1_low" else 20.0
        i, j, d = generated_lists("uniform", n, k)
    else:
        n, k, perp = 200, 30, {"perp_is_k": 30.0, "perp_one": 1.0}.get(case, 5.0)
        i, j, d = generated_lists("uniform", n, k)
        if case == "denormal":
            d = (d.astype(np.float64) * 1e-40).astype(np.float32)
            assert 0 < d.max() < np.finfo(np.float32).tiny
        elif case == "huge":
            d = (d.astype(np.float64) * 3e38).astype(np.float32)
            assert np.all(np.isfinite(d)) and d.max() > 2.9e38
    P = device_weights(i, j, d, n, perp)
    R = P.reshape(n, k)
    assert np.all(np.isfinite(P)) and np.all(P >= 0)
    assert abs(P.sum() - 1.0) < 1e-12
    assert np.allclose(R.sum(axis=1), 1.0 / n, rtol=1e-12)
    if case == "duplicates":        # beta ends at 2^256: all the weight on the nine copies
        assert np.array_equal(R[:, 9:], np.zeros((n, k - 9)))
        assert np.allclose(R[:, :9], 1.0 / (9 * n), rtol=1e-12)
    elif case in ("small_n", "equal", "all_zero", "perp_is_k"):
        assert np.allclose(P, 1.0 / (n * k), rtol=1e-12, atol=0)
    elif case in ("k1_low", "k1_high"):
        assert np.array_equal(bits(P), bits(np.full(n, 1.0 / n)))
    elif case == "perp_one":        # beta ends at 2^256: all the weight on the nearest entry
        assert np.all(R[:, 0] >= (1.0 - 1e-12) / n) and np.all(R[:, 1:] < 1e-300)
    else:
        worst = row_conditions(P, d, n, k, perp)
        print(case, worst)
        assert max(worst.values()) < 1, worst
    both(i, j, P, n, seed=5, max_iter=40 * n)


# ---- the loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(2, 1), (3, 2), (64, 8), (65, 8), (257, 16), (1000, 20)])
def test_loop_sizes(n, k):
    i, j, d, P = planted_P(n, k)
    _, st = both(i, j, P, n, seed=11, max_iter=40 * n)
    assert st["attractive"] == 40 * n and st["repulsive"] == 200 * n and st["zero_weight"] == 0
    if n <= 3:                      # a == b in about 1 / n of the pairs
        assert st["skipped"] / st["repulsive"] > 0.2, st
    else:
        assert st["skipped"] > 0, st


@pytest.mark.parametrize("n,k", [(3, 2), (257, 16)])
@pytest.mark.parametrize("n_repu", [0, 1, 127])
def test_loop_n_repu(n_repu, n, k):
    i, j, d, P = planted_P(n, k)
    _, st = both(i, j, P, n, seed=12, max_iter=40 * n, n_repu=n_repu)
    assert st["repulsive"] == n_repu * 40 * n and (st["skipped"] > 0) == (n_repu > 0)


def test_loop_eta0_zero_leaves_the_start():
    i, j, d, P = planted_P(257, 16)
    Y, st = both(i, j, P, 257, seed=13, max_iter=40 * 257, eta0=0.0)
    assert np.array_equal(bits(Y), bits(init_positions(257, 13))) and st["clipped"] == 0


@pytest.mark.parametrize("n,k", [(65, 8), (1000, 20)])
def test_loop_clips(n, k):
    """The +-0.1 clip is taken, often at eta0 = 50 and still at the default over a longer run."""
    i, j, d, P = planted_P(n, k)
    _, st = both(i, j, P, n, seed=11, max_iter=40 * n, eta0=50.0)
    assert 0.2 <= st["clipped"] / st["moved"] <= 0.95, st
    _, st = both(i, j, P, n, seed=11, max_iter=400 * n)
    assert 0.05 <= st["clipped"] / st["moved"] <= 0.5, st


@pytest.mark.parametrize("max_iter,T", [(1, 1), (2000, 2), (2500, 2), (3500, 4)])
def test_loop_schedule(max_iter, T):
    """T = 1 runs at eta0 itself, T = 2 ends at the 1e-4 floor, and half an iteration rounds to even."""
    i, j, d, P = planted_P(1000, 20)
    assert schedule(1000, max_iter) == (1000, T)
    Y, _ = both(i, j, P, 1000, seed=14, max_iter=max_iter, eta0=2.0)
    assert not np.array_equal(bits(Y), bits(init_positions(1000, 14)))


@pytest.mark.parametrize("workers", [1, 63, 64, 65, 255, 256, 257])
def test_loop_workers_round_a_wave_and_a_block(workers):
    i, j, d, P = planted_P(1000, 20)
    assert schedule(1000, 30 * workers, workers) == (workers, 30)
    _, st = both(i, j, P, 1000, seed=15, max_iter=30 * workers, workers=workers)
    assert st["attractive"] == 30 * workers


def test_loop_seeds():
    i, j, d, P = planted_P(257, 16)
    Y = {seed: both(i, j, P, 257, seed=seed, max_iter=40 * 257)[0]
         for seed in (0, 5, 1 << 63, (1 << 64) - 1, -1, (1 << 64) + 5)}
    assert np.array_equal(bits(Y[-1]), bits(Y[(1 << 64) - 1]))
    assert np.array_equal(bits(Y[(1 << 64) + 5]), bits(Y[5]))
    for a, b in ((0, 5), (0, 1 << 63), (5, 1 << 63), (0, -1)):
        assert not np.array_equal(bits(Y[a]), bits(Y[b])), (a, b)


@pytest.mark.parametrize("kind", HAND_MADE)
def test_loop_hand_made_P(kind):
    """Zero weights at the head, inside and at the tail of the prefix, and targets that hit a prefix value."""
    n, k = 257, 16
    i, j = neighbour_ring(n, k)
    P = hand_made_P(kind, n, k)
    assert (weights(P) == 0).any()
    _, st = both(i, j, P, n, seed=16, max_iter=40 * n)
    assert st["zero_weight"] == 0, st
    if kind == "unit_weights":
        assert int(weights(P).sum()) == 100 and st["exact"] > st["attractive"] // 2, st


@pytest.mark.parametrize("n,k", [(300, 10), (5000, 5)])
def test_loop_star_lists(n, k):
    """Every row lists node 0: its two delta words take an atomic from almost every attractive draw."""
    i, j = star_lists(n, k)
    both(i, j, np.full(n * k, 1.0 / (n * k)), n, seed=17, max_iter=40 * n)


def test_loop_all_weight_into_one_node():
    n, k = 5000, 5
    i, j = star_lists(n, k)
    P = np.zeros((n, k))
    P[:, 0] = 1.0 / n
    P = P.ravel()
    Y, st = both(i, j, P, n, seed=18, max_iter=20 * n, workers=n)
    assert st["attractive"] == 20 * n and st["zero_weight"] == 0
    for _ in range(2):
        assert np.array_equal(bits(device_embed(i, j, P, n, 18, 20 * n, workers=n)), bits(Y))


def test_scratch_shrinks_and_grows_on_another_stream():
    big = generated_lists("planted", 5000, 50)
    small = generated_lists("planted", 3, 2)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        Pb = device_weights(*big, 5000)
        Y1 = device_embed(big[0], big[1], Pb, 5000, seed=19, max_iter=40 * 5000)
        Ps = device_weights(*small, 3)
        both(small[0], small[1], Ps, 3, seed=19, max_iter=40 * 3)
        Pb2 = device_weights(*big, 5000)
        Y2 = device_embed(big[0], big[1], Pb2, 5000, seed=19, max_iter=40 * 5000)
    assert np.array_equal(bits(Pb), bits(Pb2)) and np.array_equal(bits(Y1), bits(Y2))
    assert np.allclose(Pb, calibrate(big[2], 5000, 50, 20.0), rtol=RTOL, atol=0)
    assert np.all(np.isfinite(Y1)) and not np.array_equal(bits(Y1), bits(init_positions(5000, 19)))


def test_host_form_agrees_with_the_device_form():
    i, j, d, P = planted_P(65, 8)
    Ph, Yh = engine.embed(i, j, d, 65, 21, perplexity=5.0, max_iter=40 * 65)
    assert np.array_equal(bits(Ph), bits(P))
    assert np.array_equal(bits(Yh), bits(both(i, j, P, 65, seed=21, max_iter=40 * 65)[0]))


# ---- arguments ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    """a good call's inputs and the restatement's answer, for the call after every refused one"""
    i, j, d = generated_lists("planted", 200, 10)
    P = calibrate(d, 200, 10, 5.0)
    return i, j, d, P, embed(P, i, j, 200, seed=22, max_iter=40 * 200)


def then_a_good_call(good):
    i, j, d, P, want = good
    assert np.allclose(device_weights(i, j, d, 200, 5.0), P, rtol=RTOL, atol=0)
    assert np.array_equal(bits(device_embed(i, j, P, 200, 22, 40 * 200)), bits(want))


@pytest.mark.parametrize("perp", [0.0, -1.0, float("nan"), float("inf")])
def test_weights_refuse_a_perplexity(good, perp):
    i, j, d, _, _ = good
    with pytest.raises(RuntimeError, match="perplexity must be finite and > 0"):
        device_weights(i, j, d, 200, perp)
    then_a_good_call(good)


@pytest.mark.parametrize("n,m", [(1, 1), (1, 0), (200, 0), (200, 200 * 200), (3, 9), (200, 1999)])
def test_sizes_refused(good, n, m):
    """n = 1, k = 0, k = n and a ragged length: the Python layer refuses them; the library says the same of n and k"""
    i = torch.zeros(m, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match=r"embed_weights_dev: lists of n\*k entries with n >= 2 and 1 <= k <= n - 1"):
        engine.embed_weights_dev(i, i, torch.zeros(m, dtype=torch.float32, device=DEV), n)
    with pytest.raises(ValueError, match=r"embed_dev: lists of n\*k entries with n >= 2 and 1 <= k <= n - 1"):
        engine.embed_dev(i, i, torch.zeros(m, dtype=torch.float64, device=DEV), n, 1)
    with pytest.raises(ValueError, match=r"embed: lists of n\*k entries"):
        engine.embed(np.zeros(m), np.zeros(m), np.zeros(m), n, 1)
    if m % n == 0:                  # the library's own check comes before it reads any array
        lib, null = _lib.lib(), C.c_void_p(None)
        text = "n must be at least 2" if n < 2 else r"k = %d must be in \[1, n - 1\]" % (m // n)
        with pytest.raises(RuntimeError, match="ppk_embed_weights: " + text):
            _lib.check(lib.ppk_embed_weights_dev(null, null, null, n, m // n, 20.0, null, null, null))
        with pytest.raises(RuntimeError, match="ppk_embed: " + text):
            _lib.check(lib.ppk_embed_dev(null, null, null, n, m // n, 1, 1000, 5, 1.0, 64, null, null))
    then_a_good_call(good)


@pytest.mark.parametrize("kw,text", [({"n_repu": -1}, r"n_repu must be in \[0, 127\]"),
                                     ({"n_repu": 128}, r"n_repu must be in \[0, 127\]"),
                                     ({"eta0": -1.0}, "eta0 must be finite and >= 0"),
                                     ({"eta0": float("nan")}, "eta0 must be finite and >= 0"),
                                     ({"eta0": float("inf")}, "eta0 must be finite and >= 0"),
                                     ({"max_iter": 0}, "max_iter must be >= 1"),
                                     ({"workers": 0}, r"workers in \[1, 2\^24\]"),
                                     ({"workers": (1 << 24) + 1}, r"workers in \[1, 2\^24\]")])
def test_loop_refuses_an_option(good, kw, text):
    i, j, d, P, _ = good
    with pytest.raises(RuntimeError, match=text):
        device_embed(i, j, P, 200, 22, **{"max_iter": 40 * 200, **kw})
    with pytest.raises(RuntimeError, match=text):
        engine.embed(i, j, d, 200, 22, **{"perplexity": 5.0, "max_iter": 40 * 200, **kw})
    then_a_good_call(good)


@pytest.mark.parametrize("case", ["all_tiny", "above_one", "negative"])
def test_loop_refuses_a_P(good, case):
    i, j, d, P, _ = good
    e = 1234
    bad = P.copy()
    if case == "all_tiny":
        bad[:] = 1e-17
        text = r"every weight rint\(P \* 2\^52\) is 0"
    else:
        bad[e] = 1.5 if case == "above_one" else -1e-300
        text = r"entry 1234 \(i = 123, j = %d\): P is %s" % (j[e], "above 1" if case == "above_one" else "negative")
    with pytest.raises(RuntimeError, match=text):
        device_embed(i, j, bad, 200, 22, 40 * 200)
    then_a_good_call(good)


def test_loop_refuses_weights_whose_sum_leaves_64_bits(good):
    """6000 entries of P = 1: the prefix of rint(P 2^52) would wrap past 2^64 and stop being monotone."""
    i, j = neighbour_ring(300, 20)
    assert int(weights(np.ones(6000)).sum()) < 6000 << 52       # the uint64 sum has wrapped
    with pytest.raises(RuntimeError, match=r"sum of the weights rint\(P \* 2\^52\) is .* below 2\^63"):
        device_embed(i, j, np.ones(6000), 300, 23, 40 * 300)
    then_a_good_call(good)
    i, j = neighbour_ring(65, 8)                                # 520 * 2^52 < 2^63: any P in [0, 1] that sums runs
    _, st = both(i, j, np.ones(520), 65, seed=23, max_iter=40 * 65)
    assert st["zero_weight"] == 0 and st["exact"] < st["attractive"]
