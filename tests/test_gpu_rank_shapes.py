"""The coded copies of a bbits = 14 database (rank-coded planes, short blocks, the folded pair) at every shape class that
reaches them.  tests/test_gpu_rank_planes.py, test_gpu_rank_short.py and test_gpu_rank_fold.py sit on s = 1024 and five
k; the route (launch_v2 behind ppk_self_job_takes_tiles) takes any database whose counts fit 64 bits: sketchsize64 1 to
156 with up to 9 k.  SHAPES holds the ends of the count-bit classes (7 to 14 bits per k, nk * bits <= 64), the flag-word
boundary on either side (31, 32 | 33 blocks: bit 31 is the last flag, 33 blocks keep no flags) and one, two and an odd
number of blocks per k (where the tile kernel fetches the next k's flag word).

Every case: option "ksplit" 0 (and "ksplit_long" 0) before the database is created, so that the self job runs whole
tiles; the random-match table on.  One related population of 100 genomes per shape, tiled to n = 257 / 300 (P = 8 and
the all-short P = 10), 1 100 (10 planes with full blocks: 513 values need 513 samples) and 2 100 (12 planes: 2^11 + 1
values).  Tiling adds no value to a position and gives every value a second holder, so D and S = D of the untouched
blocks are those of the 100; the planted positions are recounted on the CPU from the sketches.

Plantings put an exact count on either side of a threshold in ADJACENT blocks at both ends of the database -- first
block of k 0 at bit 0, last block of the last k at bit 63 -- so that a shifted or swapped flag bit, a threshold off by
one or a wrong (k, block) index changes what a block reports and, through the top plane, a match count:
  distinct(d): d values, every sample one of them in turn              -> D = d
  pairs(s):    s values with exactly two holders, the rest single      -> E = S + 2 = s + 2, D = n - s
  ENDS:        values at the ends of the presence bitmap's dwords and of the prefix sum's 32 threads

Checks: the planes and per-block planes of both codings equal the numpy model of ppk_db_create (rank_model.db_model);
the kernel that ran is the one the model names; distances and n_failed of the coded database are torch.equal to those
of "rank_planes" 0 for the whole job, a band that cuts a tile and the handle passed as its own query, under "rank_fold"
0, 1, 2 and "rank_short" 1, 0; the codes equal the numpy builder; the fused edge lists equal; the raw result meets the
CPU oracle at the bar of DESIGN.md section 5 (counts bit-exact, distances within 1e-6).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from poppunk_amd import _lib, engine, synth
from rank_model import (block_d, d_after, db_model, e_after, flags_fit, fold_codes_of, overwrite, rank_codes_of,
                        set_position, unslice)

pytestmark = pytest.mark.gpu

TOL = 1e-6          # tests/test_gpu_dist.py: distances against the CPU oracle
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")
SHAPES = [(1, 2), (1, 9), (2, 8), (3, 8), (5, 7), (31, 5), (32, 5), (33, 5), (40, 3), (64, 4), (156, 4)]
CODE_SHAPES = [(1, 9), (3, 8), (33, 5), (156, 4)]
EDGE_SHAPES = [(1, 9), (32, 5), (40, 3)]
BASE_N = 100
ENDS = [0, 31, 32, 63, 511, 512, 16351, 16352, 16383]      # first / last bit of the first / last dword and thread
RAW = "dist_kernel_v2<256x32,lds-dma>"


def kernel_name(planes, fold):
    return "dist_kernel_v2<256x32,lds-dma,rank %d%s>" % (planes, ",fold" if fold else "")


def last_kernel():
    return _lib.lib().ppk_last_kernel_name().decode()


@functools.lru_cache(maxsize=None)
def base(s64, nk):
    """the shape's 100 related genomes, their per-block D, the k list and its random-match table"""
    kmers = (13 + 2 * np.arange(nk)).astype(np.int32)
    sk = synth.make_sketches(BASE_N, kmers, sketchsize64=s64, cluster_size=10)[0]
    d = block_d(unslice(sk))
    assert d.shape == (nk, s64) and d.max() <= BASE_N
    return sk, d, kmers, synth.random_match_table(kmers)


class Planter:
    """plants exact counts into a tiled population and keeps what it claims about each position"""

    def __init__(self, s64, nk, n):
        assert n >= 2 * BASE_N          # every value of an untouched position has a second holder: S = D there
        self.sk = np.ascontiguousarray(np.tile(base(s64, nk)[0], (-(-n // BASE_N), 1, 1))[:n])
        self.blocks = [(k, b) for k in range(nk) for b in range(s64)]
        self.claims = []          # (k, block, bit, D, values with exactly two holders or None, single values or None)

    def _put(self, where, bit, vals, d, twos=None, ones=None):
        k, blk = self.blocks[where]
        set_position(self.sk, vals, k, blk, bit)
        self.claims.append((k, blk, bit, d, twos, ones))

    def distinct(self, where, bit, d):
        k, blk = self.blocks[where]
        overwrite(self.sk, k, blk, bit, d)
        self.claims.append((k, blk, bit, d, None, None))

    def pairs(self, where, bit, s):
        n = len(self.sk)
        assert n - 2 * s >= 1
        idx = np.arange(n)
        idx[:2 * s] %= s          # value i: samples i and i + s; from 2 s on a value of their own
        idx[2 * s:] -= s
        self._put(where, bit, idx * 7 + 5, n - s, s, n - 2 * s)

    def ends(self, where, bit):
        self._put(where, bit, np.asarray(ENDS)[np.arange(len(self.sk)) % len(ENDS)], len(ENDS))

    def straddle(self, plant, lo):
        """`lo` (at the threshold) and lo + 1 (past it) in adjacent blocks, at both ends of the database"""
        if len(self.blocks) >= 4:
            plant(0, 0, lo + 1)
            plant(1, 63, lo)
            plant(-1, 63, lo + 1)
            plant(-2, 0, lo)
        else:
            plant(-1, 63, lo + 1)
            plant(0, 0, lo)

    def counts(self, s64, nk):
        """per-block D and E of the planted population; every claim recounted from the sketches"""
        touched = set()
        for k, blk, bit, d, twos, ones in self.claims:
            col = unslice(self.sk[:, k:k + 1, blk * 14:(blk + 1) * 14])[:, 0, bit]
            holders = np.unique(col, return_counts=True)[1]
            assert len(holders) == d
            if twos is not None:
                assert int((holders == 2).sum()) == twos and int((holders == 1).sum()) == ones and twos + ones == d
            touched.add((k, blk))
        base_d = base(s64, nk)[1]
        return d_after(self.sk, base_d, sorted(touched)), e_after(self.sk, base_d + 2, sorted(touched))


def mid(p):
    return len(p.blocks) // 2


def plant_d8(p):
    p.straddle(p.distinct, 128)
    p.distinct(mid(p), 17, 256)
    p.ends(len(p.blocks) // 3, 5)


def plant_d10s(p):
    p.distinct(-1, 63, 257)
    p.distinct(0, 0, 256)


def plant_e8(p):
    p.straddle(p.pairs, 126)
    p.ends(len(p.blocks) // 3, 5)


def plant_d10(p):
    p.straddle(p.distinct, 512)
    p.distinct(mid(p), 17, 1024)


def plant_e8of10(p):
    p.pairs(mid(p), 17, 254)
    p.straddle(p.pairs, 126)


def plant_e10(p):
    p.pairs(mid(p), 17, 255)
    p.straddle(p.pairs, 510)


def plant_d12(p):
    p.straddle(p.distinct, 2048)
    p.distinct(mid(p), 17, 1025)


def plant_e10of12(p):
    p.pairs(mid(p), 17, 1022)
    p.straddle(p.pairs, 510)


def plant_e12(p):
    p.pairs(mid(p), 17, 1023)


# name: (n, planting, rank_planes, fold_planes under "rank_fold" 1 where flags are kept / where not, under 2)
PLANTINGS = {
    "d8": (300, plant_d8, 8, 0, 0, 8),                   # D 128 | 129 and 256: 8 planes, short and full
    "d10s": (257, plant_d10s, 10, 8, 8, 8),              # D 256 | 257: 10 planes, every block short; the pair folds to 8
    "e8": (300, plant_e8, 8, 8, 0, 8),                   # E 128 | 129: the pair wins one plane in the blocks at 128
    "d10": (1100, plant_d10, 10, 0, 0, 10),              # D 512 | 513 and 1 024
    "e8of10": (1100, plant_e8of10, 10, 8, 8, 8),         # E 256 (D 846): 8 planes folded where ranks take 10
    "e10": (1100, plant_e10, 10, 10, 0, 10),             # E 257, 512 | 513
    "d12": (2100, plant_d12, 12, 12, 0, 12),             # D 2 048 | 2 049, 1 024 | 1 025
    "e10of12": (2100, plant_e10of12, 12, 10, 10, 10),    # E 1 024 (D 1 078): 10 planes folded where ranks take 12
    "e12": (2100, plant_e12, 12, 0, 0, 12),              # E 1 025: 12 planes folded, every block short
}


def planted(s64, nk, name):
    n, plant = PLANTINGS[name][:2]
    p = Planter(s64, nk, n)
    plant(p)
    d, e = p.counts(s64, nk)
    return p.sk, d, e


class DB:
    """a database created under the given options; the options stay in force for its jobs"""

    def __init__(self, ppk_option, sk, s64, rank, fold=1):
        ppk_option("ksplit", 0)
        ppk_option("ksplit_long", 0)
        ppk_option("rank_planes", rank)
        ppk_option("rank_fold", fold)
        ppk_option("rank_short", 1)
        self.db = engine.SketchDB(sk, s64, 14)

    def __enter__(self):
        return self.db

    def __exit__(self, *exc):
        self.db.close()


def jobs(n):
    """the whole triangle, a band that cuts the 32-row query tiles, the handle as its own query"""
    return [("whole", False, {}), ("band", False, dict(q_begin=37, q_end=n - 40)), ("itself", True, {})]


def run(db, kmers, tbl, itself, band):
    out, failed = engine.dist(db, db if itself else None, kmers, tbl, **band)
    torch.cuda.synchronize()
    return out, failed, last_kernel()


def check_planes(db, d, e, fold):
    """the database against the model of ppk_db_create; returns the kernel a self job and a job of the handle against
    itself must run (the folded pair serves the triangle alone; a database that holds only the pair has no injective
    copy, and the rectangle reads the raw planes)"""
    p, blocks, pf, fblocks = db_model(d, e, fold)
    assert db.rank_planes == p and np.array_equal(db.rank_block_planes(), blocks)
    assert db.fold_planes == pf
    if pf:
        assert np.array_equal(db.fold_block_planes(), fblocks)
        return kernel_name(pf, True), RAW
    with pytest.raises(RuntimeError):
        db.fold_block_planes()
    return kernel_name(p, False), kernel_name(p, False)


@pytest.mark.parametrize("name", sorted(PLANTINGS))
@pytest.mark.parametrize("s64,nk", SHAPES)
def test_coded_route_same_bits(ppk_option, s64, nk, name):
    n, _, want_p, want_f1, want_f1_noflags, want_f2 = PLANTINGS[name]
    _, _, kmers, tbl = base(s64, nk)
    sk, d, e = planted(s64, nk, name)
    # the planting reaches the state it is named for (not read from the code under test)
    assert db_model(d, e, 0)[0] == want_p
    assert db_model(d, e, 1)[2] == (want_f1 if flags_fit(nk, s64) else want_f1_noflags)
    assert db_model(d, e, 2)[2] == want_f2
    if flags_fit(nk, s64) and name not in ("d10s", "e12"):
        mixed = db_model(d, e, 2)[1 if name.startswith("d") else 3]
        assert len(np.unique(mixed)) == 2          # a word with short and full blocks
    raw = {}
    with DB(ppk_option, sk, s64, 0) as db:
        assert db.rank_planes == 0 and db.fold_planes == 0
        for job, itself, band in jobs(n):
            out, failed, kernel = run(db, kmers, tbl, itself, band)
            assert kernel == RAW, (job, kernel)
            raw[job] = (out.clone(), failed.clone())
        if name == "d10s":          # once per shape, at the smaller n: the raw result against the CPU oracle
            counts = engine.dist(db, None, kmers, None, random_correct=False, counts=True)[0]
            assert np.array_equal(counts.cpu().numpy(), oracle.match_counts(sk, None, s64, 14, threads=4))
            want, wf = oracle.query(sk, None, kmers, s64, 14, tbl, threads=4)
            assert int(raw["whole"][1].item()) == wf
            assert np.abs(raw["whole"][0].cpu().numpy() - want).max() <= TOL
    for fold in (0, 1, 2):
        with DB(ppk_option, sk, s64, 1, fold) as db:
            self_kernel, itself_kernel = check_planes(db, d, e, fold)
            for short in (1, 0):
                ppk_option("rank_short", short)
                for job, itself, band in jobs(n):
                    out, failed, kernel = run(db, kmers, tbl, itself, band)
                    assert kernel == (itself_kernel if itself else self_kernel), (fold, short, job, kernel)
                    assert torch.equal(out, raw[job][0]) and torch.equal(failed, raw[job][1]), (fold, short, job)


@pytest.mark.parametrize("name", ["d8", "e8"])
@pytest.mark.parametrize("s64,nk", CODE_SHAPES)
def test_codes_against_numpy(ppk_option, s64, nk, name):
    """the injective codes and the folded pair ("rank_fold" 2: built at every shape), value for value; then the handle
    against itself reads the injective copy that rank_codes() built"""
    _, _, kmers, tbl = base(s64, nk)
    sk, d, e = planted(s64, nk, name)
    bins = unslice(sk)
    with DB(ppk_option, sk, s64, 0) as db:
        ref, ref_failed, _ = run(db, kmers, tbl, True, {})
        ref, ref_failed = ref.clone(), ref_failed.clone()
    with DB(ppk_option, sk, s64, 1, 2) as db:
        check_planes(db, d, e, 2)
        assert db.rank_planes == 8 and db.fold_planes == 8
        fold_r, fold_q = db.fold_codes(0), db.fold_codes(1)
        inj = db.rank_codes()
        out, failed, kernel = run(db, kmers, tbl, True, {})
        assert kernel == kernel_name(8, False)
        assert torch.equal(out, ref) and torch.equal(failed, ref_failed)
    want_r, want_q = fold_codes_of(bins)
    assert np.array_equal(inj, rank_codes_of(bins))
    assert np.array_equal(fold_r, want_r) and np.array_equal(fold_q, want_q)


@pytest.mark.parametrize("name,fold", [("d8", 0), ("e8", 1), ("e8", 2)])
@pytest.mark.parametrize("s64,nk", EDGE_SHAPES)
def test_fused_edge_lists(ppk_option, s64, nk, name, fold):
    """MODE_MASK (line boundary) and MODE_BGMM on the coded database against "rank_planes" 0"""
    from poppunk_amd.models import BGMMModel
    g = np.load(GOLDEN, allow_pickle=False)
    m = BGMMModel(g["k2_weights"], g["k2_means"], g["k2_covariances"], g["k2_scale"], g["k2_within"].item(),
                  g["k2_between"].item())
    _, _, kmers, tbl = base(s64, nk)
    sk, d, e = planted(s64, nk, name)

    def lists(db, kernel):
        got = []
        for call in (lambda: engine.dist_edges(db, None, kmers, tbl, slope=2, x_max=x_max, y_max=y_max),
                     lambda: engine.dist_bgmm_edges(db, None, kmers, tbl, model=m.model)):
            edges, failed = call()
            torch.cuda.synchronize()
            assert last_kernel() == kernel
            got.append((edges.cpu().numpy(), int(failed.item())))
        return got

    with DB(ppk_option, sk, s64, 0) as db:
        dist = engine.dist(db, None, kmers, tbl)[0].cpu().numpy()
        x_max, y_max = synth.boundary_for_quantile(dist, 0.1)
        ref = lists(db, RAW)
    assert 0 < len(ref[0][0]) < len(dist)
    with DB(ppk_option, sk, s64, 1, fold) as db:
        got = lists(db, check_planes(db, d, e, fold)[0])
    for (ge, gf), (re_, rf) in zip(got, ref):
        assert np.array_equal(ge, re_) and gf == rf
