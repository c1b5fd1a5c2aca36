"""Rank-coded resident databases (PPK_CODING_RANK): a self job that compares 8, 10 or 12 code planes per 64-bin block
must return the bits the 14 raw planes return.

Every case runs engine.dist twice on the same sketches -- option "rank_planes" 1 and 0 at database creation -- with
s = 1024, five k, the random-match correction on and option "ksplit" 0, so that these small jobs run the whole-tile
kernel (the one kernel that reads the coded copy), and requires torch.equal on the [n_pairs, 2] matrix and on n_failed.

The populations: synth.make_sketches re-uses few values per bin (at 300 genomes D, the most distinct values any
(k, bin) position holds, stays below 256); genomes with uniformly random bins add one value each to nearly every
position.  Where a case needs a D that the model does not give at its size, the sketches are put together from those
two kinds; test_thresholds_of_d tiles 200 related genomes to 4 200 (D <= 200 everywhere) before it overwrites one
position, because 4 200 genomes drawn from the model hold more than 256 values per position on their own.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from poppunk_amd import engine, synth
from rank_model import distinct_max, planes_for, unslice

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
TOL = 1e-6          # tests/test_gpu_dist.py: distances against the CPU oracle


def random_bins(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 1 << 14, size=(n, 5, 1024), dtype=np.uint16)


@pytest.fixture(scope="module")
def tbl1():
    return synth.random_match_table(KMERS)


@pytest.fixture(scope="module")
def sk300():
    return synth.make_sketches(300, KMERS)[0]


@pytest.fixture(scope="module")
def sk700():
    """450 related genomes, a copy of genome 3 (count 1 024 at every k: the wrap to the sentinel row) and 249 genomes of
    random bins (unrelated to everything: failed fits)."""
    sk = np.concatenate([synth.make_sketches(450, KMERS)[0], synth.bitslice(random_bins(250, 5), 14)])
    sk[450] = sk[3]
    return sk


def run(ppk_option, sk, tbl, rank, clusters=None, **band):
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", rank)
    db = engine.SketchDB(sk, 16, 14, clusters=clusters)
    try:
        planes = db.rank_planes
        out, failed = engine.dist(db, None, KMERS, tbl, **band)
        torch.cuda.synchronize()
        return out.clone(), failed.clone(), planes
    finally:
        db.close()


def both(ppk_option, sk, tbl, want_planes, **kw):
    got, gf, planes = run(ppk_option, sk, tbl, 1, **kw)
    ref, rf, off = run(ppk_option, sk, tbl, 0, **kw)
    assert planes == want_planes and off == 0
    assert torch.equal(got, ref) and torch.equal(gf, rf)
    return got, gf


def test_8_planes_and_oracle(ppk_option, sk300, tbl1):
    """n = 300: one full 256 tile with its diagonal and half tiles, and a strip; also against the CPU oracle"""
    assert planes_for(distinct_max(unslice(sk300))) == 8
    got, gf = both(ppk_option, sk300, tbl1, 8)
    want, wf = oracle.query(sk300, None, KMERS, 16, 14, tbl1, threads=4)
    assert int(gf.item()) == wf
    assert np.abs(got.cpu().numpy() - want).max() <= TOL


def test_10_planes(ppk_option, sk700, tbl1):
    d = distinct_max(unslice(sk700))
    assert 256 < d <= 1024
    got, gf = both(ppk_option, sk700, tbl1, 10)
    n = len(sk700)
    row = 3 * n - 3 * 4 // 2 + (450 - 3 - 1)          # condensed row of the pair (3, 450): identical genomes
    assert float(got[row].abs().max()) <= TOL
    assert int(gf.item()) > 0                          # the random genomes' fits fail


def test_10_planes_band(ppk_option, sk700, tbl1):
    both(ppk_option, sk700, tbl1, 10, q_begin=100, q_end=600)


def test_10_planes_three_clusters(ppk_option, sk700):
    rng = np.random.Generator(np.random.PCG64(11))
    tbl = synth.random_match_table(KMERS, n_clu=3)
    tbl = (tbl * rng.uniform(0.5, 3.0, size=tbl.shape)).astype(np.float32)
    clu = (np.arange(len(sk700)) % 3).astype(np.uint16)
    both(ppk_option, sk700, tbl, 10, clusters=clu)


def test_12_planes(ppk_option, tbl1):
    bins = random_bins(1500, 9)
    d = distinct_max(bins)
    assert 1024 < d <= 4096
    both(ppk_option, synth.bitslice(bins, 14), tbl1, 12)


@pytest.fixture(scope="module")
def sk4200():
    return np.ascontiguousarray(np.tile(synth.make_sketches(200, KMERS)[0], (21, 1, 1)))


@pytest.mark.parametrize("d,planes", [(256, 8), (257, 10), (1024, 10), (1025, 12), (4096, 12), (4097, 0)])
def test_thresholds_of_d(ppk_option, sk4200, tbl1, d, planes):
    """one (k, bin) position overwritten to hold exactly d distinct values; 4 097: no coded copy, the raw path"""
    sk = sk4200.copy()
    k, pos = 2, 64 * 5 + 37
    vals = (np.arange(len(sk)) % d).astype(np.uint64) * np.uint64(3) + np.uint64(1)       # d distinct 14-bit values
    assert vals.max() < (1 << 14) and len(np.unique(vals)) == d
    bit = np.uint64(pos % 64)
    for b in range(14):
        w = sk[:, k, (pos // 64) * 14 + b]
        sk[:, k, (pos // 64) * 14 + b] = (w & ~(np.uint64(1) << bit)) | (((vals >> np.uint64(b)) & np.uint64(1)) << bit)
    assert distinct_max(unslice(sk)) == d
    both(ppk_option, sk, tbl1, planes)


def test_off_switch_builds_nothing(ppk_option, sk300):
    ppk_option("ksplit", 0)
    raw_bytes = 512 * 5 * 16 * 14 * 8          # the resident raw planes of 300 genomes (padded to 512)
    deltas = {}
    for rank in (0, 0, 1):          # (the first round only warms up what a first database leaves behind)
        ppk_option("rank_planes", rank)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        db = engine.SketchDB(sk300, 16, 14)
        try:
            torch.cuda.synchronize()
            deltas[rank] = free0 - torch.cuda.mem_get_info()[0]
            assert db.rank_planes == (8 if rank else 0)
        finally:
            db.close()
    # off: the raw planes alone (device allocations are rounded up to 2 MiB); on: 8/14 of them again
    assert raw_bytes <= deltas[0] < raw_bytes + (2 << 20)
    assert deltas[1] >= deltas[0] + raw_bytes * 8 // 14


def test_small_job_on_the_ksplit_route_builds_nothing(ppk_option, sk300):
    """under the default options 300 genomes run the k-split units, which read raw planes: no copy is paid for"""
    ppk_option("rank_planes", 1)
    db = engine.SketchDB(sk300, 16, 14)
    try:
        assert db.rank_planes == 0
    finally:
        db.close()


def test_code_builder_against_numpy(ppk_option, sk300):
    """equal values have equal codes, different values different codes, every code below 2^P"""
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", 1)
    db = engine.SketchDB(sk300, 16, 14)
    try:
        assert db.rank_planes == 8
        codes = db.rank_codes()
    finally:
        db.close()
    vals = unslice(sk300)
    assert codes.shape == vals.shape and int(codes.max()) < (1 << 8)

    def n_distinct(a):
        s = np.sort(a, axis=0)
        return 1 + (s[1:] != s[:-1]).sum(axis=0)

    pairs = vals.astype(np.uint32) << 16 | codes
    nv = n_distinct(vals)
    assert np.array_equal(n_distinct(pairs), nv) and np.array_equal(n_distinct(codes), nv)
