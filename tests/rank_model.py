"""Shared numpy models of the coded copies of a bbits = 14 database (ppk_db_create, rank_code_kernel), for
tests/test_gpu_rank_planes.py, test_gpu_rank_short.py, test_gpu_rank_fold.py and test_gpu_rank_shapes.py: the sketches'
bin values, D (distinct values) and S (values with at least two holders) per position, the planes and the per-block
planes a database must report, the codes themselves, and the helpers that plant exact counts at one position."""
import numpy as np

SHORT_WORDS = 16      # PPK_RANK_SHORT_WORDS: flags are kept for nk below this and sketchsize64 <= 32 (a word per k)


def unslice(sk, bbits=14):
    """bit-sliced words [n, nk, s64 * bbits] -> bin values [n, nk, 64 * s64] (inverse of synth.bitslice)"""
    n, nk, words = sk.shape
    s64 = words // bbits
    bits = np.unpackbits(np.ascontiguousarray(sk).view(np.uint8).reshape(n, nk, s64, bbits, 8), axis=-1, bitorder="little")
    vals = np.zeros((n, nk, s64, 64), dtype=np.uint16)
    for b in range(bbits):
        vals |= bits[:, :, :, b].astype(np.uint16) << b
    return vals.reshape(n, nk, 64 * s64)


def n_distinct(a):
    """D per position: the distinct values over the samples (axis 0)"""
    s = np.sort(a, axis=0)
    return 1 + (s[1:] != s[:-1]).sum(axis=0)


def distinct_max(bins):
    """D: the most distinct values any (k, bin) position holds over the samples"""
    return int(n_distinct(bins).max())


def n_shared(bins):
    """S per position: the values at least two samples hold there (runs of equal values in the sorted column)"""
    s = np.sort(bins, axis=0)
    eq = s[1:] == s[:-1]
    starts = eq.copy()
    starts[1:] &= ~eq[:-1]
    return starts.sum(axis=0)


def shared_mask(bins):
    """per sample and position: does another sample hold the same value there"""
    order = np.argsort(bins, axis=0, kind="stable")
    s = np.take_along_axis(bins, order, axis=0)
    eq = s[1:] == s[:-1]
    m = np.zeros(s.shape, dtype=bool)
    m[1:] |= eq
    m[:-1] |= eq
    out = np.empty_like(m)
    np.put_along_axis(out, order, m, axis=0)
    return out


def block_max(per_position):
    """a figure per position [nk, 64 * s64] -> its maximum per (k, 64-bin block) [nk, s64]"""
    return per_position.reshape(per_position.shape[0], -1, 64).max(axis=2)


def block_d(bins):
    """bin values [n, nk, 64 * s64] -> the most distinct values any position of each (k, 64-bin block) holds"""
    return block_max(n_distinct(bins))


def planes_for(codes):
    return 8 if codes <= 256 else 10 if codes <= 1024 else 12 if codes <= 4096 else 0


def flags_fit(nk, s64):
    """whether a database of this shape keeps per-block flags at all: one 32-bit word per k, SHORT_WORDS - 1 words"""
    return nk < SHORT_WORDS and s64 <= 32


def planes_of(d):
    """what rank_block_planes() must say: per-block D [nk, s64] -> P from the largest, P - 1 where D <= 2^(P-1); a shape
    without flags (sketchsize64 > 32) reports P in every block"""
    p = planes_for(int(d.max()))
    short = (d <= (1 << (p - 1))) & flags_fit(*d.shape)
    return p, np.where(short, p - 1, p).astype(np.uint8)


def fold_planes_of(bins):
    """what fold_planes and fold_block_planes() must say: E = S + 2 per position, its maximum per 64-bin block and over
    all; P from the largest, P - 1 in the blocks whose E <= 2^(P-1)"""
    return planes_of(block_max(n_shared(bins) + 2))


def db_model(d, e, rank_fold):
    """ppk_db_create's choice from the per-block maxima D and E = S + 2 [nk, s64] under option "rank_fold":
    (rank_planes, rank block planes, fold_planes, fold block planes); no pair: fold_planes 0 and None.  The pair is built
    with "rank_fold" 2 always and with 1 where it compares fewer planes summed over the blocks."""
    p, blocks = planes_of(d)
    pf, fblocks = planes_of(e)
    assert p and pf          # (these tests stay below 4 097 values per position)
    if rank_fold == 2 or (rank_fold == 1 and int(fblocks.sum()) < int(blocks.sum())):
        return p, blocks, pf, fblocks
    return p, blocks, 0, None


def _sorted_columns(bins):
    """bin values [n, ...] -> per position (rows, samples last and contiguous) the sort order and the sorted values"""
    cols = np.ascontiguousarray(bins.reshape(len(bins), -1).T)
    order = np.argsort(cols, axis=1, kind="stable")
    return order, np.take_along_axis(cols, order, axis=1)


def _unsorted(codes, order, shape):
    out = np.empty_like(codes)
    np.put_along_axis(out, order, codes, axis=1)
    return np.ascontiguousarray(out.T).reshape(shape)


def rank_codes_of(bins):
    """the injective copy: per position the rank of a sample's value among the position's distinct values"""
    order, s = _sorted_columns(bins)
    rank = np.zeros(s.shape, dtype=np.uint16)
    rank[:, 1:] = np.cumsum(s[:, 1:] != s[:, :-1], axis=1)
    return _unsorted(rank, order, bins.shape)


def fold_codes_of(bins):
    """the folded pair (ref side, query side): a value with one holder is 0 on the ref side and 1 on the query side, a
    shared value 2 + its rank among the position's shared values on both"""
    order, s = _sorted_columns(bins)
    eq = s[:, 1:] == s[:, :-1]
    shared = np.zeros(s.shape, dtype=bool)
    shared[:, 1:] |= eq
    shared[:, :-1] |= eq
    start = np.ones(s.shape, dtype=bool)
    start[:, 1:] = ~eq
    code = (1 + np.cumsum(start & shared, axis=1)).astype(np.uint16)      # 2 + (shared runs begun so far - 1)
    return (_unsorted(np.where(shared, code, 0).astype(np.uint16), order, bins.shape),
            _unsorted(np.where(shared, code, 1).astype(np.uint16), order, bins.shape))


def set_position(sk, vals, k, blk, bit):
    """position (k, 64 * blk + bit) of sample i gets the 14-bit value vals[i]"""
    vals = np.asarray(vals, dtype=np.uint64)
    assert vals.shape == (len(sk),) and vals.max() < (1 << 14)
    bit = np.uint64(bit)
    for b in range(14):
        w = sk[:, k, blk * 14 + b]
        sk[:, k, blk * 14 + b] = (w & ~(np.uint64(1) << bit)) | (((vals >> np.uint64(b)) & np.uint64(1)) << bit)


def overwrite(sk, k, blk, bit, d):
    """position (k, 64 * blk + bit) gets exactly d distinct 14-bit values (as test_thresholds_of_d does)"""
    vals = (np.arange(len(sk)) % d).astype(np.uint64) * np.uint64(3) + np.uint64(1)
    assert vals.max() < (1 << 14) and len(np.unique(vals)) == d
    set_position(sk, vals, k, blk, bit)


def d_after(sk, base_d, blocks):
    """per-block D of a population whose D was base_d before the blocks in `blocks` were overwritten: those blocks are
    recomputed from the sketches' unsliced bins, the others have not changed"""
    d = base_d.copy()
    for k, blk in blocks:
        d[k, blk] = block_d(unslice(sk[:, k:k + 1, blk * 14:(blk + 1) * 14]))[0, 0]
    return d


def e_after(sk, base_e, blocks):
    """d_after for E = S + 2"""
    e = base_e.copy()
    for k, blk in blocks:
        e[k, blk] = block_max(n_shared(unslice(sk[:, k:k + 1, blk * 14:(blk + 1) * 14])) + 2)[0, 0]
    return e
