"""Numpy model of the holder pair of a bbits = 14 database (PPK_CODING_FOLDH, options "rank_foldh",
"foldh_holders", "foldh_min_planes"), for tests/test_rank_foldh_host.py and tests/test_gpu_rank_foldh.py: every value
with at most H holders at its position is coded 0 / 1, the values with more keep codes 2 + rank; the positions of a k
are sorted by E_H = (values with more than H holders) + 2; what a (pair, k) is owed is one entry (hi, lo, k, count); and
ppk_db_create's choice of H."""
import numpy as np

from rank_fold2_model import MAX_NK, MIN_ROUNDS, holders
from rank_sort_model import order_of

LADDER = (4, 8, 16, 32, 64, 128, 256)
MAX_CODES = 16         # PPK_FOLDH_MAX_CODES: codes a sorted block may span (4 planes)
SLOTS = 1024           # PPK_FOLDH_SLOTS: shared values per position
PAYS = 0.6             # the stream plane sum must be at most this share of the two-holder pair's


def held_of(bins):
    """[n, nk, nbins]: the number of samples that hold the sample's value at the position"""
    order, _, held = holders(bins)
    out = np.empty_like(held)
    np.put_along_axis(out, order, held, axis=1)
    return np.ascontiguousarray(out.T).reshape(bins.shape)


def position_eh(bins, h):
    """E_H per position [nk, nbins]: (values with more than h holders) + 2"""
    _, start, held = holders(bins)
    return (start & (held > h)).sum(axis=1).reshape(bins.shape[1:]) + 2


def block_planes(eh, order):
    """[nk, nbins / 64]: 2 where the widest position of a block of slots spans at most 4 codes, 3 at most 8, else 4;
    None where a block spans more than MAX_CODES (the pair is not built)"""
    widest = np.take_along_axis(eh, order.astype(np.int64), axis=1).reshape(eh.shape[0], -1, 64).max(axis=2)
    if widest.max() > MAX_CODES:
        return None
    return np.where(widest <= 4, 2, np.where(widest <= 8, 3, 4)).astype(np.uint8)


def stream_planes(eh, order, min_planes=2, rank_short=1):
    """what a self job compares per block under the options ("foldh_min_planes" 3, 4: never fewer; "rank_short" 0: 4)"""
    planes = block_planes(eh, order)
    return np.maximum(planes, min_planes if rank_short else 4).astype(np.uint8)


def foldh_codes_of(bins, h):
    """(ref side, query side): a value with more than h holders is 2 + its rank among the position's such values on
    both sides, every other value 0 on the ref side and 1 on the query side"""
    order, start, held = holders(bins)
    coded = held > h
    code = (1 + np.cumsum(start & coded, axis=1)).astype(np.uint16)

    def unsorted(c):
        out = np.empty_like(c)
        np.put_along_axis(out, order, c, axis=1)
        return np.ascontiguousarray(out.T).reshape(bins.shape)
    return unsorted(np.where(coded, code, 0).astype(np.uint16)), unsorted(np.where(coded, code, 1).astype(np.uint16))


def entries_of(bins, h):
    """what the compare of the two copies misses: int64 [entries, 4] of (hi, lo, k, count), hi > lo, one per (pair, k)
    that shares values with 2 .. h holders, count the number of positions at which it does; sorted by (k, hi, lo).
    Per k the incidence matrix A (folded value x sample) gives the counts as the strict lower triangle of A^T A."""
    from scipy import sparse
    n, nk, nbins = bins.shape
    order, start, held = holders(bins)
    run = np.cumsum(start, axis=1) - 1
    out = []
    for k in range(nk):
        rows = slice(k * nbins, (k + 1) * nbins)
        folded = (held[rows] >= 2) & (held[rows] <= h)
        value = (run[rows] + np.arange(nbins)[:, None] * n)[folded]       # a key per (position, value)
        a = sparse.csr_matrix((np.ones(len(value), dtype=np.int32), (value, order[rows][folded])), shape=(nbins * n, n))
        owed = sparse.tril(a.T @ a, k=-1).tocoo()
        out.append(np.stack([owed.row, owed.col, np.full(owed.nnz, k), owed.data], axis=1).astype(np.int64))
    ent = np.concatenate(out)
    return ent[np.lexsort((ent[:, 1], ent[:, 0], ent[:, 2]))]


def owed_brute(bins, h):
    """the same by brute force, dense [n (hi), n (lo), nk] (small populations)"""
    held = held_of(bins)
    folded = (held >= 2) & (held <= h)
    n, nk, _ = bins.shape
    out = np.zeros((n, n, nk), dtype=np.int64)
    for i in range(n):
        out[i] = ((bins[i][None] == bins) & folded[i][None]).sum(axis=2)
    out[np.triu_indices(n)] = 0
    return out


def buckets_of(ent, n):
    """the counting sort of ppk_db_create: (offsets [npad / 32 * npad / 256 + 1], entries uint32 sorted within each
    bucket); bucket (lo // 32) * (npad // 256) + hi // 256, entry hi % 256 | (lo % 32) << 8 | k << 13 | count << 16"""
    npad = (n + 255) // 256 * 256
    rt, qt = npad // 256, npad // 32
    b = (ent[:, 1] // 32) * rt + ent[:, 0] // 256
    packed = ((ent[:, 0] % 256) | ((ent[:, 1] % 32) << 8) | (ent[:, 2] << 13) | (ent[:, 3] << 16)).astype(np.uint32)
    idx = np.lexsort((packed, b))
    off = np.zeros(qt * rt + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.bincount(b, minlength=qt * rt))
    return off, packed[idx]


def max_entries(n, nk, rank_foldh=1):
    """the cap on the entries: a sixteenth of the self job's (pair, k) ("rank_foldh" 2: all of them)"""
    return n * (n - 1) // 2 * nk // (1 if rank_foldh == 2 else 16)


def choice(eh_of, fold2_sum, n, nk, s64, rank_foldh=1, foldh_holders=0, tile_slots=512):
    """ppk_db_create: the holder bound H of the pair, None for no pair -- a pure function of E_H per position
    (eh_of(h) -> [nk, nbins]), the two-holder pair's stream plane sum, the shape and the options.  (The cap on the
    entries is applied after the pair's counts are known: max_entries.)"""
    if rank_foldh == 0 or nk > MAX_NK or s64 > 32 or n >= (1 << 24):
        return None
    npad = (n + 255) // 256 * 256
    four_rounds = (npad // 256) * (npad // 32) // 2 >= MIN_ROUNDS * tile_slots
    for h in ((foldh_holders,) if foldh_holders else LADDER):
        eh = eh_of(h)
        planes = block_planes(eh, order_of(eh))
        if planes is None:
            continue
        if rank_foldh == 2 or (four_rounds and planes.sum() * 10 <= fold2_sum * 6):
            return h
    return None


def planted_holders(n, kept, h, seed, folded=4):
    """bin values [n, nk, nbins] with E_h = kept[k, pos] + 2 at every position: kept[k, pos] values with more than h
    holders (the first exactly h + 1), up to `folded` values with 2 .. h holders (the first exactly h, the second
    exactly 2), every other sample a value of its own.  The holders of a value are a run of neighbouring samples from a
    start drawn per position: a related population whose pairs are owed different counts."""
    rng = np.random.default_rng(seed)
    nk, nbins = kept.shape
    assert n + 1000 < (1 << 14) and kept.max() * (h + 3) + folded * h <= n
    bins = np.empty((n, nk, nbins), dtype=np.uint16)
    own = 1000 + np.arange(n)
    for k in range(nk):
        for pos in range(nbins):
            who = (int(rng.integers(n)) + np.arange(n)) % n
            col, at = own.copy(), 0
            for v in range(int(kept[k, pos])):
                size = h + 1 + (int(rng.integers(0, 3)) if v else 0)
                col[who[at:at + size]] = v
                at += size
            for f in range(int(rng.integers(0, folded + 1))):
                size = h if f == 0 else 2 if f == 1 else int(rng.integers(2, h + 1))
                col[who[at:at + size]] = 500 + f
                at += size
            bins[:, k, pos] = col
    return bins


def match_counts(a, b):
    """matches per (pair, k) of two code arrays [n, nk, nbins]: [n (ref), n (query), nk]"""
    out = np.zeros((len(a), len(b), a.shape[1]), dtype=np.int64)
    for i in range(len(a)):
        out[i] = (a[i][None] == b).sum(axis=2)
    return out
