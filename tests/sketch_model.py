"""The sketch rule "poppunk_amd:sketch1" (include/ppk.h "Sketching") restated in numpy: hash, bin,
densify, bit-slice and the per-sample statistics, every one from its definition and none from the kernel's schedule (no
rolling, no pieces).  [EXT] The rule is this project's own; it is not pinned to pp-sketchlib.

Codes: 0-3 = A, C, G, T; 4 = any other residue; 5 = contig break."""
import numpy as np

SEEDS = np.array([0x3c8bfbb395c60474, 0x3193c18562a02b4c, 0x20323ed082572324, 0x295549f54be24456], dtype=np.uint64)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def rol(x, r):
    """rotate the uint64 array x left by r (taken mod 64)"""
    r = int(r) % 64
    x = np.asarray(x, dtype=np.uint64)
    return x if r == 0 else (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def hashes(codes, k, strand_preserved=False):
    """(start positions, hash) of every valid k-mer of one sample: f = XOR_i rol(seed[s_i], k-1-i),
    r = XOR_i rol(seed[3-s_i], i), h = min(f, r) or f."""
    c = np.asarray(codes, dtype=np.uint8)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64)
    ok = c < 4
    bad = np.concatenate([[0], np.cumsum(~ok)])
    valid = (bad[k:] - bad[:-k]) == 0
    base = np.minimum(c, 3)
    sf = np.where(ok, SEEDS[base], np.uint64(0))
    sr = np.where(ok, SEEDS[3 - base], np.uint64(0))
    f = np.zeros(n, dtype=np.uint64)
    r = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        f ^= rol(sf[i:i + n], k - 1 - i)
        r ^= rol(sr[i:i + n], i)
    h = f if strand_preserved else np.minimum(f, r)
    return np.flatnonzero(valid), h[valid]


def bin_of(h, nbins):
    """floor(h * nbins / 2^64) for nbins < 2^32, in 64-bit pieces"""
    h = np.asarray(h, dtype=np.uint64)
    nb = np.uint64(nbins)
    hi, lo = h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)
    return ((hi * nb + ((lo * nb) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def keep(h):
    """what a bin keeps of a hash: the all-ones word marks an empty bin, so that one hash is kept one lower"""
    h = np.asarray(h, dtype=np.uint64)
    return np.where(h == EMPTY, h - np.uint64(1), h)


def minima(codes, k, nbins, strand_preserved=False):
    """uint64 [nbins]: the least kept hash of every bin, EMPTY where no k-mer fell"""
    _, h = hashes(codes, k, strand_preserved)
    m = np.full(nbins, EMPTY, dtype=np.uint64)
    np.minimum.at(m, bin_of(h, nbins), keep(h))
    return m


def densify(m, bbits=14):
    """(bin values int64 [nbins], filled): the low bbits of every minimum; an empty bin takes the value of the nearest
    non-empty bin above it, cyclically, in the state before densification.  filled == 0: all zero."""
    m = np.asarray(m, dtype=np.uint64)
    full = np.flatnonzero(m != EMPTY)
    if full.size == 0:
        return np.zeros(len(m), dtype=np.int64), 0
    src = full[np.searchsorted(full, np.arange(len(m))) % full.size]
    return (m[src] & np.uint64((1 << bbits) - 1)).astype(np.int64), int(full.size)


def bitslice(values, bbits=14):
    """bin values [64 * s64] -> uint64 [s64 * bbits]: word [blk * bbits + b] = bit b of bins 64 blk .. 64 blk + 63"""
    v = np.asarray(values, dtype=np.uint64).reshape(-1, 64)
    out = np.zeros((v.shape[0], bbits), dtype=np.uint64)
    for lane in range(64):
        for b in range(bbits):
            out[:, b] |= ((v[:, lane] >> np.uint64(b)) & np.uint64(1)) << np.uint64(lane)
    return out.reshape(-1)


def stats(codes):
    """[length, missing bases, A, C, G, T]"""
    c = np.asarray(codes, dtype=np.uint8)
    return np.array([int((c < 5).sum()), int((c == 4).sum())] + [int((c == x).sum()) for x in range(4)], dtype=np.int64)


def sketch(codes, seq_off, kmers, sketchsize64, bbits=14, strand_preserved=False):
    """(words uint64 [n][nk][sketchsize64 * bbits], stats int64 [n][6], filled int32 [n][nk]) of ppk_sketch"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, nk, nbins = len(seq_off) - 1, len(kmers), 64 * sketchsize64
    words = np.zeros((n, nk, sketchsize64 * bbits), dtype=np.uint64)
    st = np.zeros((n, 6), dtype=np.int64)
    filled = np.zeros((n, nk), dtype=np.int32)
    for i in range(n):
        c = codes[int(seq_off[i]):int(seq_off[i + 1])]
        st[i] = stats(c)
        for j, k in enumerate(kmers):
            values, filled[i, j] = densify(minima(c, int(k), nbins, strand_preserved), bbits)
            words[i, j] = bitslice(values, bbits)
    return words, st, filled


def jaccard(codes_a, codes_b, k, strand_preserved=False):
    """the exact Jaccard index of the two samples' sets of k-mer hashes"""
    a = np.unique(hashes(codes_a, k, strand_preserved)[1])
    b = np.unique(hashes(codes_b, k, strand_preserved)[1])
    both = np.intersect1d(a, b, assume_unique=True).size
    return both / float(a.size + b.size - both)


def equal_bins(values_a, values_b):
    return float((np.asarray(values_a) == np.asarray(values_b)).mean())


def random_genome(rng, length):
    return rng.integers(0, 4, size=length, dtype=np.uint8)


def mutate(rng, codes, pi):
    """every base replaced by a different one with probability pi"""
    c = np.array(codes, dtype=np.uint8)
    hit = rng.random(len(c)) < pi
    c[hit] = (c[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) % 4
    return c


def reverse_complement(codes):
    c = np.asarray(codes, dtype=np.uint8)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)
