"""Short blocks of a rank-coded database: a 64-bin block none of whose positions holds more than 2^(P-1) distinct values
has a zero top code plane, and a self job compares P - 1 planes there (option "rank_short", PpkCoding::less1).  The
bits must be those of the 14 raw planes.

Settings as in tests/test_gpu_rank_planes.py: s = 1024, five k, option "ksplit" 0 (whole tiles), the random-match
table on; every comparison is torch.equal (np.array_equal on edge lists) between "rank_planes" 1 with "rank_short" 1
and "rank_planes" 0, on the result and on n_failed.

Populations: 200 related genomes hold at most 50 distinct values per position, so tiled to any size every block is
short at every P; a block is made full by overwriting one of its positions with exactly d = 2^(P-1) + 1 values.  The
position then holds ranks r and r + 2^(P-1), which differ in the top plane alone: a kernel that left that plane out
there would count one match too many for those pairs.
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from poppunk_amd import engine, synth
from rank_model import block_d, d_after, overwrite, planes_of, unslice

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
TOL = 1e-6          # tests/test_gpu_dist.py: distances against the CPU oracle
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")


@pytest.fixture(scope="module")
def tbl1():
    return synth.random_match_table(KMERS)


@pytest.fixture(scope="module")
def sk200():
    return synth.make_sketches(200, KMERS)[0]


@pytest.fixture(scope="module")
def base_d(sk200):
    d = block_d(unslice(sk200))          # (tiling a population adds no value to any position)
    assert d.shape == (5, 16) and d.max() <= 64
    return d


@pytest.fixture(scope="module")
def sk4200(sk200):
    return np.ascontiguousarray(np.tile(sk200, (21, 1, 1)))


@pytest.fixture(scope="module")
def sk600(sk200):
    return np.ascontiguousarray(np.tile(sk200, (3, 1, 1)))


@pytest.fixture(scope="module")
def mixed600(sk600, base_d):
    """600 genomes, P = 8, blocks (2, 5) and (4, 15) full and the other 78 short"""
    sk = sk600.copy()
    blocks = [(2, 5), (4, 15)]
    overwrite(sk, 2, 5, 37, 129)
    overwrite(sk, 4, 15, 63, 129)
    p, want = planes_of(d_after(sk, base_d, blocks))
    assert p == 8 and int((want == 8).sum()) == 2 and want[2, 5] == 8 and want[4, 15] == 8
    return sk, want


def run(ppk_option, sk, tbl, rank, short=1, **band):
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", rank)
    ppk_option("rank_short", short)
    db = engine.SketchDB(sk, 16, 14)
    try:
        planes = db.rank_planes
        per_block = db.rank_block_planes() if planes else None
        out, failed = engine.dist(db, None, KMERS, tbl, **band)
        torch.cuda.synchronize()
        return out.clone(), failed.clone(), planes, per_block
    finally:
        db.close()


def both(ppk_option, sk, tbl, want_planes, want_blocks, **kw):
    got, gf, planes, per_block = run(ppk_option, sk, tbl, 1, **kw)
    ref, rf, off, _ = run(ppk_option, sk, tbl, 0, **kw)
    assert planes == want_planes and off == 0
    assert np.array_equal(per_block, want_blocks)
    assert torch.equal(got, ref) and torch.equal(gf, rf)
    return got, gf


def test_all_blocks_short_and_oracle(ppk_option, tbl1):
    """n = 300: P = 8 and every block compares 7 planes; a full tile with its diagonal and half tiles, and a strip"""
    sk = synth.make_sketches(300, KMERS)[0]
    p, want = planes_of(block_d(unslice(sk)))
    assert p == 8 and (want == 7).all()
    got, gf = both(ppk_option, sk, tbl1, 8, want)
    ref, rf = oracle.query(sk, None, KMERS, 16, 14, tbl1, threads=4)
    assert int(gf.item()) == rf
    assert np.abs(got.cpu().numpy() - ref).max() <= TOL


@pytest.mark.parametrize("d,planes,full", [(128, 8, False), (129, 8, True), (512, 10, False), (513, 10, True),
                                           (2048, 12, False), (2049, 12, True)])
def test_flag_boundary(ppk_option, sk4200, base_d, tbl1, d, planes, full):
    """d = 2^(P-1): every block short; d = 2^(P-1) + 1: exactly block (2, 5) full"""
    sk = sk4200.copy()
    overwrite(sk, 2, 5, 37, d)
    p, want = planes_of(d_after(sk, base_d, [(2, 5)]))
    assert p == planes
    assert int((want == planes).sum()) == (1 if full else 0) and (want[2, 5] == planes) == full
    both(ppk_option, sk, tbl1, planes, want)


@pytest.mark.parametrize("blocks", [[(0, 0)], [(2, 5)], [(4, 15)], [(0, 0), (4, 15)], [(1, 15), (2, 0)]])
def test_flag_indexing(ppk_option, sk600, base_d, tbl1, blocks):
    """the full block at the first, a middle and the last (k, block); two full blocks in one database"""
    sk = sk600.copy()
    for i, (k, blk) in enumerate(blocks):
        overwrite(sk, k, blk, (11 + 26 * i) % 64, 129)
    p, want = planes_of(d_after(sk, base_d, blocks))
    assert p == 8 and sorted(zip(*np.nonzero(want == 8))) == sorted(blocks)
    both(ppk_option, sk, tbl1, 8, want)


def test_band(ppk_option, mixed600, tbl1):
    sk, want = mixed600
    both(ppk_option, sk, tbl1, 8, want, q_begin=100, q_end=500)


def test_rank_short_off_same_bits_same_flags(ppk_option, mixed600, tbl1):
    """option "rank_short" 0: every block takes the full stream; the database's flags are still reported"""
    sk, want = mixed600
    on, onf, p1, blocks1 = run(ppk_option, sk, tbl1, 1, short=1)
    off, offf, p0, blocks0 = run(ppk_option, sk, tbl1, 1, short=0)
    raw, rawf, _, _ = run(ppk_option, sk, tbl1, 0)
    assert p1 == 8 and p0 == 8
    assert np.array_equal(blocks1, want) and np.array_equal(blocks0, want)
    assert torch.equal(on, raw) and torch.equal(onf, rawf)
    assert torch.equal(off, raw) and torch.equal(offf, rawf)


def edges(ppk_option, sk, tbl, rank, call):
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", rank)
    ppk_option("rank_short", 1)
    db = engine.SketchDB(sk, 16, 14)
    try:
        planes = db.rank_planes
        e, failed = call(db)
        torch.cuda.synchronize()
        return e.cpu().numpy(), int(failed.item()), planes
    finally:
        db.close()


def test_fused_edge_list(ppk_option, mixed600, tbl1):
    """MODE_MASK on the mixed database"""
    sk, _ = mixed600
    d, _, _, _ = run(ppk_option, sk, tbl1, 0)
    x_max, y_max = synth.boundary_for_quantile(d.cpu().numpy(), 0.1)

    def call(db):
        return engine.dist_edges(db, None, KMERS, tbl1, slope=2, x_max=x_max, y_max=y_max)
    got, gf, planes = edges(ppk_option, sk, tbl1, 1, call)
    ref, rf, off = edges(ppk_option, sk, tbl1, 0, call)
    assert planes == 8 and off == 0
    assert 0 < len(ref) < len(d)
    assert np.array_equal(got, ref) and gf == rf


def test_fused_bgmm_assignment(ppk_option, mixed600, tbl1):
    """MODE_BGMM on the mixed database"""
    from poppunk_amd.models import BGMMModel
    g = np.load(GOLDEN, allow_pickle=False)
    m = BGMMModel(g["k2_weights"], g["k2_means"], g["k2_covariances"], g["k2_scale"], g["k2_within"].item(),
                  g["k2_between"].item())
    sk, _ = mixed600

    def call(db):
        return engine.dist_bgmm_edges(db, None, KMERS, tbl1, model=m.model)
    got, gf, planes = edges(ppk_option, sk, tbl1, 1, call)
    ref, rf, off = edges(ppk_option, sk, tbl1, 0, call)
    assert planes == 8 and off == 0
    assert np.array_equal(got, ref) and gf == rf
