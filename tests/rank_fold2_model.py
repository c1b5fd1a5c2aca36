"""Numpy model of the two-holder pair of a bbits = 14 database (PPK_CODING_FOLD2, option "rank_fold2"), for
tests/test_rank_fold2_host.py and tests/test_gpu_rank_fold2.py: per position the holders of every value, D / S / S3 and
E2 = S3 + 2, the codes of the two copies, the events (hi, lo, k) the tile kernel adds back, their buckets, the caps and
ppk_db_create's choice among the three codings."""
import numpy as np

from rank_model import SHORT_WORDS, block_max, planes_of

SLOTS = 256            # PPK_FOLD2_SLOTS: two-holder values per position
MAX_PER_PAIR = 63      # PPK_FOLD2_MAX_PER_PAIR: events per (pair, k)
MAX_NK = 5             # PPK_FOLD2_MAX_NK
MIN_ROUNDS = 4         # the default builds the pair only for a self job of at least this many rounds of tiles


def holders(bins):
    """bin values [n, nk, nbins] -> per position (rows = (k, bin), samples sorted by value): the sort order, whether an
    entry starts a run of equal values, and the number of samples that hold the entry's value"""
    n = len(bins)
    cols = np.ascontiguousarray(bins.reshape(n, -1).T)
    order = np.argsort(cols, axis=1, kind="stable")
    s = np.take_along_axis(cols, order, axis=1)
    start = np.ones(s.shape, dtype=bool)
    start[:, 1:] = s[:, 1:] != s[:, :-1]
    run = np.cumsum(start, axis=1) - 1
    rows = np.repeat(np.arange(len(s)), n).reshape(s.shape)
    length = np.zeros(s.shape, dtype=np.int64)
    np.add.at(length, (rows, run), 1)
    return order, start, np.take_along_axis(length, run, axis=1)


def counts_of(bins):
    """per position [nk, nbins]: D (distinct values), S (at least two holders), S3 (at least three), T = S - S3"""
    _, start, held = holders(bins)
    shape = bins.shape[1:]
    d = start.sum(axis=1).reshape(shape)
    s = (start & (held >= 2)).sum(axis=1).reshape(shape)
    s3 = (start & (held >= 3)).sum(axis=1).reshape(shape)
    return d, s, s3, s - s3


def block_counts(bins):
    """what rank_counts() must report: the per-block maxima of D, E = S + 2, E2 = S3 + 2, the most two-holder values of
    a position and their number"""
    d, s, s3, t = counts_of(bins)
    return block_max(d), block_max(s + 2), block_max(s3 + 2), int(t.max()), int(t.sum())


def fold2_codes_of(bins):
    """(ref side, query side): a value with at least three holders is 2 + its rank among the position's such values on
    both sides, every other value 0 on the ref side and 1 on the query side"""
    order, start, held = holders(bins)
    coded = held >= 3
    code = (1 + np.cumsum(start & coded, axis=1)).astype(np.uint16)

    def unsorted(c):
        out = np.empty_like(c)
        np.put_along_axis(out, order, c, axis=1)
        return np.ascontiguousarray(out.T).reshape(bins.shape)
    return unsorted(np.where(coded, code, 0).astype(np.uint16)), unsorted(np.where(coded, code, 1).astype(np.uint16))


def events_of(bins):
    """one event per value with exactly two holders: int64 [events, 3] of (hi, lo, k), hi > lo the holders"""
    order, start, held = holders(bins)
    nbins = bins.shape[2]
    row, col = np.nonzero(start & (held == 2))
    a, b = order[row, col], order[row, col + 1]
    return np.stack([np.maximum(a, b), np.minimum(a, b), row // nbins], axis=1).astype(np.int64)


def per_pair_max(ev):
    """the most events any (pair, k) holds"""
    if not len(ev):
        return 0
    return int(np.unique(ev, axis=0, return_counts=True)[1].max())


def buckets_of(ev, n):
    """the counting sort of ppk_db_create: (offsets [npad / 32 * npad / 256 + 1], events uint16 sorted within each
    bucket); bucket (lo // 32) * (npad // 256) + hi // 256, event hi % 256 | (lo % 32) << 8 | k << 13"""
    npad = (n + 255) // 256 * 256
    rt, qt = npad // 256, npad // 32
    b = (ev[:, 1] // 32) * rt + ev[:, 0] // 256
    packed = ((ev[:, 0] % 256) | ((ev[:, 1] % 32) << 8) | (ev[:, 2] << 13)).astype(np.uint16)
    idx = np.lexsort((packed, b))
    off = np.zeros(qt * rt + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.bincount(b, minlength=qt * rt))
    return off, packed[idx]


def sorted_buckets(off, ev):
    """a device list with every bucket sorted (the scatter's order within a bucket is not fixed)"""
    out = ev.copy()
    for i in np.nonzero(off[1:] > off[:-1])[0]:
        out[off[i]:off[i + 1]] = np.sort(ev[off[i]:off[i + 1]])
    return out


def plane_sum(block_codes):
    """the planes a self job compares over all blocks under a coding with these per-block code counts (no coding: 14)"""
    p, blocks = planes_of(block_codes)
    return (int(blocks.sum()) if p else 14 * block_codes.size), p


def choice(bd, be, be2, two_max, pair_max, n, rank_fold=1, rank_fold2=1, tile_slots=512):
    """ppk_db_create: which coding a self job reads -- "fold2", "fold" or "rank" -- from the per-block maxima [nk, s64]"""
    nk = bd.shape[0]
    (sum_d, p), (sum_e, pf), (sum_e2, pf2) = plane_sum(bd), plane_sum(be), plane_sum(be2)
    npad = (n + 255) // 256 * 256
    fits = pf2 == 8 and nk <= MAX_NK and two_max <= SLOTS and pair_max <= MAX_PER_PAIR and n < (1 << 28)
    pays = (rank_fold != 0 and sum_e2 < sum_d and (not pf or sum_e2 < sum_e)
            and (npad // 256) * (npad // 32) // 2 >= MIN_ROUNDS * tile_slots)
    if fits and rank_fold2 != 0 and (rank_fold2 == 2 or pays):
        return "fold2"
    if pf and rank_fold != 0 and (rank_fold == 2 or sum_e < sum_d):
        return "fold"
    return "rank" if p else "raw"


def match_counts(a, b):
    """matches per (pair, k) of two code arrays [n, nk, nbins]: [n (ref), n (query), nk]"""
    return (a[:, None] == b[None, :]).sum(axis=3)


assert SHORT_WORDS > MAX_NK      # (the two-holder pair always keeps its per-block flags where sketchsize64 <= 32)
