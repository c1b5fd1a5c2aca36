"""The rule for sketching read sets (include/ppk.h "Sketching read sets") restated in numpy, from its
definition and with none of the kernels' schedule: counts by np.unique, the count table by np.bincount per row, the
admitted minima, the four integers per (sample, k) and the length estimate.  The hash, the bin, what a bin keeps,
densify and bit-slicing are sketch_model's.  [EXT] Rows, remix and default bits of the table are this project's own.

Codes: 0-3 = A, C, G, T; 4 = any other residue; 5 = contig break (between reads)."""
import numpy as np

import sketch_model as sm

ROWS = 2
MULT = (np.uint64(0x9e3779b97f4a7c15), np.uint64(0xc2b2ae3d27d4eb4f))
BITS_MIN, BITS_MAX = 4, 26


def count_index(h, row, bits):
    """row `row`'s counter of the kept hashes h: (h ^ (h >> 29)) * MULT[row] mod 2^64, cut to its top `bits` bits"""
    h = np.asarray(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        m = (h ^ (h >> np.uint64(29))) * MULT[row]
    return (m >> np.uint64(64 - bits)).astype(np.int64)


def count_bits(codes):
    """the default bits of a sample of `codes` codes: ceil(log2(codes)) + 2 within 12 .. 26"""
    b = 0
    while b < BITS_MAX and (1 << b) < codes:
        b += 1
    return min(max(b + 2, 12), BITS_MAX)


def kept_hashes(codes, k, strand_preserved=False):
    """the kept hash of every valid start position of one sample, in order"""
    return sm.keep(sm.hashes(codes, k, strand_preserved)[1])


def exact_counts(h):
    """per occurrence, the number of occurrences with the same kept hash"""
    _, inverse, counts = np.unique(h, return_inverse=True, return_counts=True)
    return counts[inverse.reshape(-1)] if len(h) else np.zeros(0, dtype=np.int64)


def table_admits(h, min_count, bits):
    """per occurrence: every one of its ROWS counters (each the sum of the counts of the hashes that index it) is at
    least min_count"""
    ok = np.ones(len(h), dtype=bool)
    for row in range(ROWS):
        idx = count_index(h, row, bits)
        ok &= np.bincount(idx, minlength=1 << bits)[idx] >= min_count
    return ok


def admitted_minima(h, nbins, min_count, exact, bits):
    """(minima uint64 [nbins], kstats [occ, adm_occ, filled, win_occ]) from one sample's kept hashes.  adm_occ is the
    count table's verdict on both routes (all occurrences at min_count 1); the minima are over the k-mers the route
    admits."""
    m = np.full(nbins, sm.EMPTY, dtype=np.uint64)
    if len(h) == 0:
        return m, np.zeros(4, dtype=np.int64)
    counts = exact_counts(h)
    table = table_admits(h, min_count, bits) if min_count > 1 else np.ones(len(h), dtype=bool)
    admitted = (counts >= min_count) if (exact and min_count > 1) else table
    bins = sm.bin_of(h, nbins)
    np.minimum.at(m, bins[admitted], h[admitted])
    win_occ = int((h == m[bins]).sum())                         # every occurrence of a bin's winner: the winners' counts
    filled = int((m != sm.EMPTY).sum())
    return m, np.array([len(h), int(table.sum()), filled, win_occ], dtype=np.int64)


def length_estimate(adm_occ, filled, win_occ):
    """adm_occ * filled / win_occ rounded half up; 0 when nothing was admitted"""
    if win_occ == 0 or filled == 0:
        return 0
    return (2 * int(adm_occ) * int(filled) + int(win_occ)) // (2 * int(win_occ))


def sketch_reads(codes, seq_off, kmers, sketchsize64, min_count, exact=False, bits=0, bbits=14, strand_preserved=False,
                 hashes=None):
    """(words uint64 [n][nk][sketchsize64 * bbits], stats int64 [n][6], kstats int64 [n][nk][4], filled int32 [n][nk])
    of ppk_sketch_reads.  bits 0: the default of every sample.  hashes: {(sample, k): kept hashes}, computed already."""
    codes = np.asarray(codes, dtype=np.uint8)
    n, nk, nbins = len(seq_off) - 1, len(kmers), 64 * sketchsize64
    words = np.zeros((n, nk, sketchsize64 * bbits), dtype=np.uint64)
    st = np.zeros((n, 6), dtype=np.int64)
    kst = np.zeros((n, nk, 4), dtype=np.int64)
    filled = np.zeros((n, nk), dtype=np.int32)
    largest = int(np.argmax(np.asarray(kmers)))                 # (the first of the largest k)
    for i in range(n):
        c = codes[int(seq_off[i]):int(seq_off[i + 1])]
        st[i] = sm.stats(c)
        b = bits if bits else count_bits(len(c))
        for j, k in enumerate(kmers):
            h = hashes[(i, int(k))] if hashes is not None else kept_hashes(c, int(k), strand_preserved)
            m, kst[i, j] = admitted_minima(h, nbins, min_count, exact, b)
            values, filled[i, j] = sm.densify(m, bbits)
            words[i, j] = sm.bitslice(values, bbits)
        st[i, 0] = length_estimate(kst[i, largest, 1], kst[i, largest, 2], kst[i, largest, 3])
    return words, st, kst, filled


def simulate_reads(rng, genome, coverage, read_len=100, error=0.01, n_share=0.02):
    """(codes, read count): reads of a circular genome at uniform starts, every base substituted with probability
    `error`, half of the reads reverse-complemented, a share n_share of them carrying one N; a code 5 between reads"""
    g = np.asarray(genome, dtype=np.uint8)
    n_reads = int(round(coverage * len(g) / read_len))
    starts = rng.integers(0, len(g), size=n_reads)
    reads = g[(starts[:, None] + np.arange(read_len)[None, :]) % len(g)]
    hit = rng.random(reads.shape) < error
    reads[hit] = (reads[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) % 4
    flip = rng.random(n_reads) < 0.5
    reads[flip] = 3 - reads[flip][:, ::-1]
    with_n = np.flatnonzero(rng.random(n_reads) < n_share)
    reads[with_n, rng.integers(0, read_len, size=len(with_n))] = 4
    out = np.full((n_reads, read_len + 1), 5, dtype=np.uint8)
    out[:, :read_len] = reads
    return out.reshape(-1)[:-1].copy() if n_reads else np.zeros(0, dtype=np.uint8), n_reads


def closed_assembly(genome, k):
    """the genome plus its first k - 1 bases: the circle's k-mers as a contig"""
    g = np.asarray(genome, dtype=np.uint8)
    return np.concatenate([g, g[:k - 1]])
