"""Numpy model of the sorted positions of the two-holder pair (the order of PPK_CODING_FOLD2, options "fold2_sort" and
"fold2_min_planes"), for tests/test_rank_sort_host.py and tests/test_gpu_rank_sort.py: E2 per position, the order of a
k's positions, the planes the tile kernel compares per block of slots, the copies in slot order, and populations
planted to a chosen E2 per position."""
import numpy as np

from rank_fold2_model import counts_of


def position_e2(bins):
    """E2 = S3 + 2 per position [nk, nbins]: the codes a position of the two-holder pair spans"""
    return counts_of(bins)[2] + 2


def order_of(e2, sort=True):
    """[nk, nbins]: slot i of k holds stored position order[k, i] -- E2 descending, ties by stored position ascending;
    sort = False ("fold2_sort" 0): the identity"""
    if not sort:
        return np.tile(np.arange(e2.shape[1], dtype=np.uint32), (e2.shape[0], 1))
    return np.argsort(-e2.astype(np.int64), axis=1, kind="stable").astype(np.uint32)


def stream_planes(e2, order, min_planes=6, rank_short=1):
    """[nk, nbins / 64]: 8 where the widest position of a block of slots spans more than 128 codes, 7 above 64, else 6
    ("fold2_min_planes" 7: never below 7; "rank_short" 0: 8 everywhere).  Flags are kept for at most 32 blocks per k."""
    widest = np.take_along_axis(e2, order.astype(np.int64), axis=1).reshape(e2.shape[0], -1, 64).max(axis=2)
    planes = np.where(widest > 128, 8, np.where(widest > 64, 7, 6))
    if not rank_short or widest.shape[1] > 32:
        return np.full(widest.shape, 8, dtype=np.uint8)
    return np.maximum(planes, min_planes).astype(np.uint8)


def in_slots(codes, order):
    """codes [n, nk, nbins] in stored position order -> the same in slot order"""
    return np.stack([codes[:, k, order[k]] for k in range(codes.shape[1])], axis=1)


def planted_e2(n, targets, seed, pairs=3):
    """bin values [n, nk, nbins] with E2 = targets[k, pos] at every position: targets - 2 values with at least three
    holders each (exactly three where the target leaves no room for more), up to `pairs` values with exactly two (the
    events), every other sample a value of its own.  The holders of a value are a run of neighbouring samples, from a
    start drawn per position, so two samples share the fewer values the further apart they are: a related population,
    whose distances differ from pair to pair."""
    rng = np.random.default_rng(seed)
    nk, nbins = targets.shape
    assert targets.min() >= 2 and 3 * (targets.max() - 2) + 2 * pairs <= n and n + 1000 < (1 << 14)
    bins = np.empty((n, nk, nbins), dtype=np.uint16)
    own = 1000 + np.arange(n)
    for k in range(nk):
        for pos in range(nbins):
            t, two = int(targets[k, pos]) - 2, int(rng.integers(0, pairs + 1))
            alone = int(rng.integers(0, min(30, n - 2 * two - 3 * t) + 1)) if t else n - 2 * two
            m = n - 2 * two - alone
            who = (int(rng.integers(n)) + np.arange(n)) % n
            col = own.copy()
            if t:
                col[who[:m]] = np.repeat(np.arange(t), np.diff(np.linspace(0, m, t + 1).astype(np.int64)))
            rest = rng.permutation(who[m:])
            col[rest[:2 * two]] = 500 + np.arange(2 * two) // 2
            bins[:, k, pos] = col
    return bins


def spread_targets(nk, nbins, top, seed, wide=None):
    """E2 targets [nk, nbins]: a spread of 20 .. 64 everywhere, then per k the counts of `wide` -- a list per k of
    (E2, positions) -- at random positions; E2 <= top"""
    rng = np.random.default_rng(seed)
    t = rng.integers(20, 65, size=(nk, nbins))
    for k, spec in enumerate(wide or []):
        free = list(rng.permutation(nbins))
        for e2, count in spec:
            for _ in range(count):
                t[k, free.pop()] = e2
    assert t.max() <= top
    return t
