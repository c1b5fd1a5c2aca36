"""The embedding on the host side (poppunk_amd/mandrake.py): the numpy restatement of the rules
ppk_embed_weights_dev and ppk_embed_dev run (include/ppk.h), which the GPU tests compare against bit for bit, and
the quality that definition reaches on planted clusters.  CPU only.

calibrate() restates the calibration (P agrees with the device's to rounding: exp and log differ by ulps between
libms).  embed() restates the loop exactly: the generator, the integer sampling, the snapshot reads, the Q32.32
accumulation and the Eq fold, so that the same P and seed give the device's bits."""
import math

import numpy as np
import pytest

from poppunk_amd import mandrake, synth

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
INIT_KEY = 0xD1B54A32D192ED03
CAL_STEPS = 256
CAL_TOL = 2.0 ** -48
GAIN_CLIP = 0.1
WORKERS = 65536


# ---- the generator of ppk_embed.hip ------------------------------------------------------------------------------
def fmix(z):
    """splitmix64's finaliser, on a uint64 array."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draw(key, ctr):
    """fmix(key + (ctr + 1) * G) for uint64 counters ctr."""
    with np.errstate(over="ignore"):
        return fmix(np.uint64(key) + (np.asarray(ctr, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLDEN))


def iter_key(seed, t):
    return int(fmix(np.uint64((seed + (t + 1) * GOLDEN) & M64)))


def mulhi(r, m):
    """The high 64 bits of r * m (r uint64 array, 0 <= m < 2^64)."""
    r = np.asarray(r, dtype=np.uint64)
    lo32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    rh, rl = r >> s32, r & lo32
    mh, ml = np.uint64(int(m) >> 32), np.uint64(int(m) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        ll, lh, hl, hh = rl * ml, rl * mh, rh * ml, rh * mh
        mid = (ll >> s32) + (lh & lo32) + (hl & lo32)
        return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


# ---- the definition ----------------------------------------------------------------------------------------------
def calibrate(dist, n, k, perplexity, with_beta=False):
    """P float64 [n*k] of the lists' distances (ppk_embed_weights_dev): rms-normalised, x = d^2 - min d^2 per row,
    beta by bisection (doubling while unbounded) until hi - lo <= hi * 2^-48 or 256 steps; P = (p / Z) / n."""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64).reshape(n, k)
    ss = float(np.sum(d * d))
    rms = math.sqrt(ss / (n * k)) if ss > 0 else 1.0
    x = d / rms
    x = x * x
    x = x - x.min(axis=1, keepdims=True)
    target = math.log(perplexity)
    beta, lo, hi = np.ones(n), np.zeros(n), np.full(n, np.inf)
    done = np.zeros(n, dtype=bool)
    for _ in range(CAL_STEPS):
        act = ~done
        if not act.any():
            break
        b, xa = beta[act], x[act]
        p = np.exp(-b[:, None] * xa)
        Z = p.sum(axis=1)
        H = np.log(Z) + b * (p * xa).sum(axis=1) / Z
        up = H > target
        lo_a, hi_a = lo[act], hi[act]
        nb = np.where(up, np.where(np.isinf(hi_a), b * 2.0, (b + hi_a) / 2.0), (lo_a + b) / 2.0)
        lo_a = np.where(up, b, lo_a)
        hi_a = np.where(up, hi_a, b)
        beta[act], lo[act], hi[act] = nb, lo_a, hi_a
        done[act] = np.isfinite(hi_a) & (hi_a - lo_a <= hi_a * CAL_TOL)
    p = np.exp(-beta[:, None] * x)
    P = (p / p.sum(axis=1, keepdims=True) / n).ravel()
    return (P, beta) if with_beta else P


def weights(P):
    """The integer sampling weights c = rint(P * 2^52)."""
    return np.rint(np.asarray(P, dtype=np.float64) * 2.0 ** 52).astype(np.uint64)


def schedule(n, max_iter, workers=WORKERS):
    """(W, T): W = min(workers, n) workers per iteration -- the small-n cap -- and T = max(1, round(max_iter / W))."""
    W = min(int(workers), int(n))
    return W, max(1, round(max_iter / W))


def init_positions(n, seed):
    r = draw(int(fmix(np.uint64((seed ^ INIT_KEY) & M64))), np.arange(2 * n, dtype=np.uint64))
    return ((((r >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) * 2.0 - 1.0) * 1e-4).reshape(n, 2)


def _fixed(x):
    return np.rint(x * 2.0 ** 32).astype(np.int64)


def embed(P, i, j, n, seed, max_iter, n_repu=5, eta0=1.0, workers=WORKERS):
    """Y float64 [n, 2] of ppk_embed_dev, bit for bit."""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    prefix = np.cumsum(weights(P), dtype=np.uint64)
    total = int(prefix[-1])
    W, T = schedule(n, max_iter, workers)
    Y = init_positions(n, seed)
    Eq = 1.0
    nsq = float(n) * float(n - 1)
    w8 = np.arange(W, dtype=np.uint64) << np.uint64(8)
    for t in range(T):
        eta = eta0 * max(1.0 - t / (T - 1), 1e-4) if T > 1 else eta0
        key = iter_key(seed, t)
        e = np.searchsorted(prefix, mulhi(draw(key, w8), total), side="right")
        pairs = [(i[e], j[e])]
        for s in range(n_repu):
            pairs.append((mulhi(draw(key, w8 | np.uint64(1 + 2 * s)), n).astype(np.int64),
                          mulhi(draw(key, w8 | np.uint64(2 + 2 * s)), n).astype(np.int64)))
        delta = np.zeros((n, 2), dtype=np.int64)
        qsum = qcount = 0
        for s, (a, b) in enumerate(pairs):
            keep = a != b
            a, b = a[keep], b[keep]
            dY = Y[a] - Y[b]
            q = 1.0 / (1.0 + (dY[:, 0] * dY[:, 0] + dY[:, 1] * dY[:, 1]))
            if s == 0:
                g = -4.0 * q
            else:
                g = 4.0 * q * q / Eq
                qsum += int(_fixed(q).sum())
                qcount += int(keep.sum())
            fx = _fixed(np.clip((eta * g)[:, None] * dY, -GAIN_CLIP, GAIN_CLIP))
            np.add.at(delta, a, fx)
            np.add.at(delta, b, -fx)
        Y = Y + delta.astype(np.float64) * 2.0 ** -32
        Eq = (Eq * nsq + qsum * 2.0 ** -32) / (nsq + qcount)
    return Y


# ---- inputs and measures -----------------------------------------------------------------------------------------
def knn_lists(D, k):
    """get_kNN_distances of a square (stable order, the row itself skipped): (i, j, dist float32) of n*k."""
    D = np.asarray(D, dtype=np.float32)
    n = D.shape[0]
    M = D.copy()
    np.fill_diagonal(M, np.inf)
    jj = np.argsort(M, axis=1, kind="stable")[:, :k]
    return (np.repeat(np.arange(n, dtype=np.int64), k), jj.ravel().astype(np.int64),
            np.take_along_axis(D, jj, 1).ravel())


def planted(nc=20, size=100, dim=30, seed=1):
    """nc Gaussian clusters of `size` samples in dim dimensions: (square float32, labels)."""
    rng = np.random.default_rng(seed)
    X = np.repeat(rng.normal(0.0, 3.0, size=(nc, dim)), size, axis=0) + rng.normal(0.0, 1.0, size=(nc * size, dim))
    sq = (X * X).sum(axis=1)
    D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0)).astype(np.float32)
    np.fill_diagonal(D, 0.0)
    return D, np.repeat(np.arange(nc), size)


def embedded_neighbours(Y, k=10):
    Y = np.asarray(Y, dtype=np.float64)
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    return np.argsort(D, axis=1, kind="stable")[:, :k]


def quality(nb, labels, j, K, k=10):
    """(fraction of the k embedded neighbours in the point's cluster, overlap with its k nearest input neighbours)"""
    n = nb.shape[0]
    same = float((labels[nb] == labels[:, None]).mean())
    inp = np.asarray(j).reshape(n, K)[:, :k]
    overlap = float(np.mean([np.intersect1d(nb[r], inp[r]).size / k for r in range(n)]))
    return same, overlap


# gates (DESIGN.md 3.11 records what the restatement reaches)
SAME_GATE, OVERLAP_GATE = 0.9, 0.15


def entropy_rows(P, n, k):
    p = np.asarray(P).reshape(n, k) * n
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.sum(np.where(p > 0, p * np.log(p), 0.0), axis=1)


# ---- tests -------------------------------------------------------------------------------------------------------
def test_calibration_reaches_the_perplexity():
    D, _ = planted(nc=5, size=40)
    i, j, d = knn_lists(D, 50)
    for perp in (5.0, 20.0, 30.0):
        P = calibrate(d, 200, 50, perp)
        H = entropy_rows(P, 200, 50)
        assert np.max(np.abs(H - math.log(perp))) < 1e-9
        assert abs(P.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("case", ["duplicates", "small_n", "equal"])
def test_calibration_defined_when_unreachable(case):
    rng = np.random.default_rng(3)
    if case == "duplicates":        # 10 exact copies of every genome: 9 zero distances per row, ln 9 > ln 5
        X = np.repeat(rng.normal(size=(12, 5)), 10, axis=0)
        D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)).astype(np.float32)
        n, k, perp = 120, 20, 5.0
    elif case == "small_n":         # n = 10: K = 9 < perplexity 20
        X = rng.normal(size=(10, 3))
        D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)).astype(np.float32)
        n, k, perp = 10, 9, 20.0
    else:                           # all distances equal
        D = np.full((50, 50), 0.25, dtype=np.float32)
        n, k, perp = 50, 30, 20.0
    i, j, d = knn_lists(D, k)
    P, beta = calibrate(d, n, k, perp, with_beta=True)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(beta)) and np.all(P >= 0)
    assert abs(P.sum() - 1.0) < 1e-12
    assert np.allclose(P.reshape(n, k).sum(axis=1), 1.0 / n, rtol=1e-12)
    if case == "duplicates":        # beta ends at 2^256: all the weight on the copies
        assert np.array_equal(P.reshape(n, k)[:, 9:], np.zeros((n, k - 9)))
        assert np.allclose(P.reshape(n, k)[:, :9], 1.0 / (9 * n), rtol=1e-12)
    else:                           # uniform: nothing to tell neighbours apart
        assert np.allclose(P, 1.0 / (n * k), rtol=1e-12)
    Y = embed(P, i, j, n, seed=5, max_iter=2000)
    assert np.all(np.isfinite(Y))


def test_all_zero_distances_are_left_as_they_are():
    d = np.zeros(40 * 7, dtype=np.float32)
    P = calibrate(d, 40, 7, 3.0)
    assert np.allclose(P, 1.0 / 280, rtol=1e-12)


def test_integer_sampling_matches_the_weights():
    rng = np.random.default_rng(11)
    P = rng.random(100) ** 3
    P = P / P.sum()
    c = weights(P)
    prefix = np.cumsum(c, dtype=np.uint64)
    total = int(prefix[-1])
    assert total == sum(int(x) for x in c)
    draws = 10 ** 6
    r = draw(iter_key(123, 0), np.arange(draws, dtype=np.uint64) << np.uint64(8))
    e = np.searchsorted(prefix, mulhi(r, total), side="right")
    assert e.max() < 100
    seen = np.bincount(e, minlength=100)
    expect = draws * c.astype(np.float64) / total
    chi2 = float(((seen - expect) ** 2 / expect).sum())
    assert chi2 < 99 + 6 * math.sqrt(2 * 99)          # 99 degrees of freedom
    nodes = mulhi(r, 7).astype(np.int64)
    assert nodes.min() == 0 and nodes.max() == 6


def test_mulhi_is_the_high_word():
    rng = np.random.default_rng(2)
    r = rng.integers(0, 2 ** 63, size=1000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for m in (1, 7, 2 ** 52 + 12345, 2 ** 64 - 1):
        got = mulhi(r, m)
        want = [(int(x) * m) >> 64 for x in r]
        assert [int(g) for g in got] == want


def test_generator_is_splitmix64():
    # splitmix64 seeded with 0: its first output is fmix(G)
    assert int(draw(0, np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(fmix(np.uint64(GOLDEN))) == 0xE220A8397B1DCDAF


def test_dot_writer_matches_the_reference_expression(tmp_path):
    labels = ["a", "s 2", "x_3"]
    Y = np.array([[0.1, -2.5e-07], [1e16, 3.0], [-0.0, 1.0 / 3.0]])
    fn = str(tmp_path / "e.dot")
    mandrake.write_dot(labels, Y, fn)
    want = ('graph G { "a"[x="0.5",y="-1.2499999999999999e-06"]; "s 2"[x="5e+16",y="15.0"]; '
            '"x_3"[x="-0.0",y="1.6666666666666665"]; }\n')
    assert open(fn).read() == want


def test_file_name_and_existing_file(tmp_path, capsys):
    out = tmp_path / "run"
    out.mkdir()
    fn = str(out / "run_perplexity20_accessory_mandrake.dot")
    open(fn, "w").write("kept")
    got = mandrake.generate_embedding(["a", "b"], np.zeros((2, 2), dtype=np.float32), 20, str(out), False)
    assert got == fn and open(fn).read() == "kept"
    assert "already exists" in capsys.readouterr().err


def test_schedule_caps_the_workers():
    assert schedule(2000, 10 ** 7) == (2000, 5000)
    assert schedule(10 ** 6, 10 ** 7) == (65536, 153)
    assert schedule(3, 10) == (3, 3)
    assert schedule(5000, 12500) == (5000, 2)             # round half to even
    assert schedule(5000, 1) == (5000, 1)


@pytest.mark.parametrize("n", [2, 3])
def test_tiny_n(n):
    X = np.arange(n, dtype=np.float64)[:, None] * np.array([[1.0, 0.5]])
    D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)).astype(np.float32)
    k = min(50, n - 1)
    i, j, d = knn_lists(D, k)
    P = calibrate(d, n, k, 20.0)
    Y = embed(P, i, j, n, seed=9, max_iter=1000)
    assert Y.shape == (n, 2) and np.all(np.isfinite(Y))


def test_planted_clusters_quality_at_65536_requested_workers():
    """The divergence case of uncapped workers (n = 2000, W = 65 536 requested): the cap W = n holds it."""
    D, labels = planted()
    i, j, d = knn_lists(D, 50)
    P = calibrate(d, 2000, 50, 20.0)
    Y = embed(P, i, j, 2000, seed=7, max_iter=10 ** 6, workers=65536)
    assert np.all(np.isfinite(Y)) and np.abs(Y).max() < 100
    same, overlap = quality(embedded_neighbours(Y), labels, j, 50)
    assert same >= SAME_GATE and overlap >= OVERLAP_GATE, (same, overlap)


def test_synthetic_population_quality():
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, labels = synth.make_sketches(1000, kmers, cluster_size=50, seed=5)
    dist, _ = oracle.query(sk, None, kmers, 16, 14, random_tbl=synth.random_match_table(kmers),
                           threads=oracle.max_threads())
    acc = oracle.long_to_square(dist[:, 1])
    K = 50
    i, j, d = knn_lists(acc, K)
    P = calibrate(d, 1000, K, 20.0)
    Y = embed(P, i, j, 1000, seed=13, max_iter=10 ** 6)
    same, overlap = quality(embedded_neighbours(Y), labels, j, K)
    assert same >= SAME_GATE and overlap >= OVERLAP_GATE, (same, overlap)
