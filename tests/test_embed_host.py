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
    beta by bisection (doubling while unbounded) until hi - lo <= hi * 2^-48 or 256 steps (k <= perplexity: beta =
    2^-256 at once); P = (p / Z) / n."""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64).reshape(n, k)
    ss = float(np.sum(d * d))
    rms = math.sqrt(ss / (n * k)) if ss > 0 else 1.0
    x = d / rms
    x = x * x
    x = x - x.min(axis=1, keepdims=True)
    target = math.log(perplexity)
    beta, lo, hi = np.ones(n), np.zeros(n), np.full(n, np.inf)
    done = np.zeros(n, dtype=bool)
    if perplexity >= k:             # unreachable: beta = 2^-256, where 256 halvings end, without asking H
        beta[:] = 2.0 ** -256
        done[:] = True
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


STATS = ("moved", "clipped", "repulsive", "skipped", "attractive", "zero_weight", "exact")


def embed(P, i, j, n, seed, max_iter, n_repu=5, eta0=1.0, workers=WORKERS, stats=None):
    """Y float64 [n, 2] of ppk_embed_dev, bit for bit.  A dict passed as `stats` receives what the run did (counts
    over all iterations; Y does not depend on it): coordinates `moved` (two per pair that was not skipped) and of
    those `clipped` (|eta g dY| > 0.1 before the clip); `repulsive` pairs drawn and of those `skipped` for a == b;
    `attractive` draws, of those on a `zero_weight` entry (c == 0: never, by the upper bound) and with a target
    that equalled a prefix value exactly (`exact`: where > and >= in the search differ)."""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    c = weights(P)
    prefix = np.cumsum(c, dtype=np.uint64)
    total = int(prefix[-1])
    W, T = schedule(n, max_iter, workers)
    Y = init_positions(n, seed)
    Eq = 1.0
    nsq = float(n) * float(n - 1)
    w8 = np.arange(W, dtype=np.uint64) << np.uint64(8)
    if stats is not None:
        stats.update(dict.fromkeys(STATS, 0))
    for t in range(T):
        eta = eta0 * max(1.0 - t / (T - 1), 1e-4) if T > 1 else eta0
        key = iter_key(seed, t)
        x = mulhi(draw(key, w8), total)
        e = np.searchsorted(prefix, x, side="right")
        if stats is not None:
            at = np.minimum(np.searchsorted(prefix, x, side="left"), prefix.size - 1)
            stats["attractive"] += W
            stats["zero_weight"] += int((c[e] == 0).sum())
            stats["exact"] += int((prefix[at] == x).sum())
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
            gain = (eta * g)[:, None] * dY
            if stats is not None:
                stats["moved"] += gain.size
                stats["clipped"] += int((np.abs(gain) > GAIN_CLIP).sum())
                if s:
                    stats["repulsive"] += keep.size
                    stats["skipped"] += int(keep.size - keep.sum())
            fx = _fixed(np.clip(gain, -GAIN_CLIP, GAIN_CLIP))
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


def row_conditions(P, dist, n, k, perplexity):
    """What a calibrated P must satisfy whichever libm evaluated exp and log: the largest
    observed / allowed ratio over the rows of each condition, {"sum", "beta", "entropy"}; all must be < 1.
    Evaluated in np.longdouble from float64 x = (d / rms)^2 - min (rms from numpy: its last-ulp difference from the
    device's fixed-order sum rescales x uniformly, which beta-hat absorbs).  Per row, p = n P:
      sum      |sum p - 1| <= (k + 4) 2^-53;
      beta     over the entries with x > 0 and p > 2^-1000, beta-hat = -ln(p_j / p_min) / x_j at the largest such x
               (p_min: p at the row's minimum); |ln(p_j / p_min) + beta-hat x_j| <= 16 2^-53 (1 + beta-hat x_j) for
               each of them: one beta made the whole row, to the error of exp and the product's rounding;
      entropy  rows that can reach the target (ln #entries at the minimum < ln perplexity < ln k):
               |H(p) - ln perplexity| <= Var_p(ln p) 2^-47 + (k + 16) 2^-52, the bisection's 2^-48 bracket through
               H'(beta) = -beta Var(x), doubled, plus summation noise."""
    ld = np.longdouble
    d = np.asarray(dist, dtype=np.float32).astype(np.float64).reshape(n, k)
    ss = float(np.sum(d * d))
    rms = math.sqrt(ss / (n * k)) if ss > 0 else 1.0
    x = d / rms
    x = x * x
    x = x - x.min(axis=1, keepdims=True)
    p = np.asarray(P, dtype=np.float64).reshape(n, k).astype(ld) * ld(n)
    target = ld(math.log(perplexity))
    worst = {"sum": 0.0, "beta": 0.0, "entropy": 0.0}
    worst["sum"] = float(np.max(np.abs(p.sum(axis=1) - ld(1)) / (ld(k + 4) * ld(2.0) ** -53)))
    for r in range(n):
        xr, pr = x[r], p[r]
        at_min = xr == 0
        use = (xr > 0) & (pr > ld(2.0) ** -1000)
        if use.any():
            xs = xr[use].astype(ld)
            lr = np.log(pr[use] / pr[np.argmax(at_min)])
            far = np.argmax(xs)
            bx = -lr[far] / xs[far] * xs
            worst["beta"] = max(worst["beta"], float(np.max(np.abs(lr + bx) / (ld(16) * ld(2.0) ** -53 * (1 + bx)))))
        if math.log(int(at_min.sum())) < target < math.log(k):
            pos = pr[pr > 0]
            lp = np.log(pos)
            H = -np.sum(pos * lp)
            var = np.sum(pos * lp * lp) - H * H
            allowed = var * ld(2.0) ** -47 + ld(k + 16) * ld(2.0) ** -52
            worst["entropy"] = max(worst["entropy"], float(abs(H - target) / allowed))
    return worst


GENERATORS = ("uniform", "wide", "one_near", "planted")


def neighbour_ring(n, k):
    """(i, j) of valid lists: row r lists r + 1 .. r + k (mod n)."""
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    return i, (i + 1 + np.tile(np.arange(k, dtype=np.int64), n)) % n


def generated_lists(kind, n, k, seed=1):
    """(i, j, dist float32) of n*k entries, every row ascending: `uniform` U(0, 1); `wide` 10^U(-6, 1), seven
    decades (rows with H(beta) nearly flat, beta ill-conditioned); `one_near` two entries U(0, 1e-3) and the rest
    U(5, 40); `planted` the k nearest neighbours in planted() clusters (well-conditioned rows)."""
    if kind == "planted":
        size = 100 if n >= 200 else (n + 1) // 2
        D, _ = planted(nc=max(2, -(-n // size)), size=size, seed=seed)
        return knn_lists(D[:n, :n], k)
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        d = rng.random((n, k))
    elif kind == "wide":
        d = 10.0 ** rng.uniform(-6.0, 1.0, size=(n, k))
    elif kind == "one_near":
        d = rng.uniform(5.0, 40.0, size=(n, k))
        d[:, :2] = rng.uniform(0.0, 1e-3, size=(n, min(2, k)))
    else:
        raise ValueError(kind)
    i, j = neighbour_ring(n, k)
    return i, j, np.sort(d.astype(np.float32), axis=1).ravel()


HARD_SHAPES = [(n, k, perp) for n, k in ((200, 30), (130, 129), (1025, 7)) for perp in (1.5, 5.0, 20.0) if perp < k]

HAND_MADE = ("first_row_zero", "last_row_zero", "half_zero", "single", "unit_weights")


def hand_made_P(kind, n, k, seed=1):
    """P float64 [n*k] with zero weights where the prefix search has to step over them, sum 1 (but `unit_weights`:
    P = 2^-52 on 100 random entries, 0 elsewhere, so every c is 0 or 1, the total 100 and every target but 0 equals
    a prefix value)."""
    rng = np.random.default_rng(seed)
    m = n * k
    if kind == "unit_weights":
        P = np.zeros(m)
        P[rng.choice(m, 100, replace=False)] = 2.0 ** -52
        return P
    P = rng.random(m) + 0.1
    if kind == "first_row_zero":
        P[:k] = 0.0
    elif kind == "last_row_zero":
        P[-k:] = 0.0
    elif kind == "half_zero":
        P[rng.random(m) < 0.5] = 0.0
        P[:3] = 0.0
        P[-3:] = 0.0
    elif kind == "single":
        P[:] = 0.0
        P[m // 3] = 1.0
    else:
        raise ValueError(kind)
    return P / P.sum()


def star_lists(n, k):
    """(i, j): every row lists node 0 first (row 0: node 1), then the next nodes round the ring that are neither."""
    j = np.empty((n, k), dtype=np.int64)
    for r in range(n):
        first = 0 if r else 1
        rest = [v % n for v in range(r + 1, r + k + 3) if v % n not in (r, first)]
        j[r] = [first] + rest[:k - 1]
    return np.repeat(np.arange(n, dtype=np.int64), k), j.ravel()


def run_stats(P, i, j, n, **kw):
    st = {}
    Y = embed(P, i, j, n, stats=st, **kw)
    return Y, st


# ---- tests -------------------------------------------------------------------------------------------------------
def test_stats_leave_the_bits_alone():
    i, j, d = generated_lists("planted", 257, 16)
    P = calibrate(d, 257, 16, 20.0)
    plain = embed(P, i, j, 257, seed=3, max_iter=40 * 257)
    Y, st = run_stats(P, i, j, 257, seed=3, max_iter=40 * 257)
    assert np.array_equal(plain.view(np.int64), Y.view(np.int64))
    assert set(st) == set(STATS)
    assert st["attractive"] == 40 * 257 and st["repulsive"] == 5 * 40 * 257
    assert st["moved"] == 2 * (st["attractive"] + st["repulsive"] - st["skipped"])
    assert st["zero_weight"] == 0 and 0 < st["skipped"] < st["repulsive"] // 50


@pytest.mark.parametrize("kind", GENERATORS)
def test_restatement_stays_inside_the_row_conditions(kind):
    for n, k, perp in HARD_SHAPES:
        i, j, d = generated_lists(kind, n, k)
        assert np.all(np.diff(d.reshape(n, k), axis=1) >= 0) and np.all(j != i) and j.min() >= 0 and j.max() < n
        worst = row_conditions(calibrate(d, n, k, perp), d, n, k, perp)
        print(kind, n, k, perp, worst)
        assert max(worst.values()) < 1, (kind, n, k, perp, worst)


def test_row_conditions_notice_a_wrong_row():
    n, k, perp = 200, 30, 5.0
    _, _, d = generated_lists("uniform", n, k)
    P = calibrate(d, n, k, perp).reshape(n, k)
    assert max(row_conditions(P, d, n, k, perp).values()) < 1
    bent = P.copy()
    bent[7, 3] *= 1.0 + 1e-13                       # one entry off its row's beta by 1e-13
    assert row_conditions(bent, d, n, k, perp)["beta"] > 1
    other = calibrate(d, n, k, perp * (1.0 + 1e-10)).reshape(n, k)    # every row a valid Gibbs row of another target
    worst = row_conditions(other, d, n, k, perp)
    assert worst["beta"] < 1 and worst["sum"] < 1 and worst["entropy"] > 1
    short = P.copy()
    short[11] *= 1.0 - 1e-13
    assert row_conditions(short, d, n, k, perp)["sum"] > 1
    unscaled = calibrate(d * np.float32(1024.0), n, k, perp)          # the scale of the distances does not matter
    assert max(row_conditions(unscaled, d, n, k, perp).values()) < 1


def test_shares_the_device_tests_rely_on():
    """The clip, skip and exact-hit shares of the cases tests/test_gpu_embed_shapes.py names, from calibrate()'s P
    (the device's differs by ulps; the windows do not notice)."""
    i, j, d = generated_lists("planted", 3, 2)
    _, st = run_stats(calibrate(d, 3, 2, 20.0), i, j, 3, seed=11, max_iter=40 * 3)
    assert st["repulsive"] == 600 and st["skipped"] / st["repulsive"] > 0.2, st
    i, j, d = generated_lists("planted", 2, 1)
    _, st = run_stats(calibrate(d, 2, 1, 20.0), i, j, 2, seed=11, max_iter=40 * 2)
    assert st["skipped"] / st["repulsive"] > 0.2, st
    for n, k in ((65, 8), (1000, 20)):
        i, j, d = generated_lists("planted", n, k)
        P = calibrate(d, n, k, 5.0)
        _, st = run_stats(P, i, j, n, seed=11, max_iter=40 * n, eta0=50.0)
        assert 0.2 <= st["clipped"] / st["moved"] <= 0.95, (n, st)
        _, st = run_stats(P, i, j, n, seed=11, max_iter=400 * n)
        assert 0.05 <= st["clipped"] / st["moved"] <= 0.5, (n, st)
    i, j = neighbour_ring(257, 16)
    for kind in HAND_MADE:
        _, st = run_stats(hand_made_P(kind, 257, 16), i, j, 257, seed=11, max_iter=40 * 257)
        assert st["zero_weight"] == 0, (kind, st)
    assert st["exact"] > st["attractive"] // 2, st                    # unit_weights, the last one


def test_star_lists_are_valid():
    for n, k in ((300, 10), (5000, 5)):
        i, j = star_lists(n, k)
        J = j.reshape(n, k)
        assert np.all(J[1:, 0] == 0) and J[0, 0] == 1 and np.all(j != i) and j.min() >= 0 and j.max() < n
        assert all(len(set(row)) == k for row in J[:50])


def test_calibration_reaches_the_perplexity():
    D, _ = planted(nc=5, size=40)
    i, j, d = knn_lists(D, 50)
    for perp in (5.0, 20.0, 30.0):
        P = calibrate(d, 200, 50, perp)
        H = entropy_rows(P, 200, 50)
        assert np.max(np.abs(H - math.log(perp))) < 1e-9
        assert abs(P.sum() - 1.0) < 1e-12


def unreachable_case(case):
    """(square float32, n, k, perplexity) of a row set whose target entropy cannot be reached."""
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
    return D, n, k, perp


@pytest.mark.parametrize("case", ["duplicates", "small_n", "equal"])
def test_calibration_defined_when_unreachable(case):
    D, n, k, perp = unreachable_case(case)
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


def test_perplexity_at_k_is_uniform():
    """K <= perplexity takes beta = 2^-256 at once: at K == perplexity H is within rounding of the target up to
    beta ~ 1e-8 and a bisection that asked it ended 3e-8 from uniform, by the last bit of log."""
    _, _, d = generated_lists("uniform", 200, 30)
    for perp in (30.0, 31.0, 1e6):
        P, beta = calibrate(d, 200, 30, perp, with_beta=True)
        assert np.all(beta == 2.0 ** -256) and np.allclose(P, 1.0 / 6000, rtol=1e-12, atol=0)
    H = entropy_rows(calibrate(d, 200, 30, 29.0), 200, 30)
    assert np.max(np.abs(H - math.log(29.0))) < 1e-9


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
