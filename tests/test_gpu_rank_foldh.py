"""The holder pair (options "rank_foldh", "foldh_holders", "foldh_min_planes"): every bin value with at most H holders is
coded 0 / 1, the positions of a k are sorted by the codes left, a block of slots compares 4, 3 or 2 planes, and the tile
kernel adds what each (pair, k) is owed from the database's entries.

Populations are planted to a chosen number of values with more than H holders per position (tests/foldh_model.py: the
first of them exactly H + 1 holders, then a few values with 2 .. H holders -- the first exactly H, the second exactly 2
-- and every other sample a value of its own; holders are runs of neighbouring samples, so pairs are owed different
counts):
  n = 400, sketchsize64 16, H 4:  blocks of 4, 3 and 2 planes, a different mix per k; samples 17 and 390 are duplicates,
                                  owed nearly 1 024 at every k (the two-holder pair's field stops at 63)
  n = 400, sketchsize64 3, H 4:   the three blocks of k 0 compare 4, 3 and 2 planes
  n = 257, sketchsize64 8, H 4:   the second ref tile holds one sample
  n = 400, sketchsize64 16, H 64: at most three values with more than 64 holders; most pairs are owed something
Both ref tiles of n = 400 end in a strip (144 samples past the last whole tile), n = 257 is nearly all strip.
Checks: H, order, stream planes, codes and entries equal the model; distances and n_failed are torch.equal for the whole
job, a band that cuts a tile and the handle as its own query under "foldh_min_planes" 3 and 4, "rank_short" 0,
"rank_foldh" 0 (the two-holder pair), "rank_fold2" 0 (the folded pair) and "rank_planes" 0 (the raw planes, whose
counts and distances meet the CPU oracle); both fused edge lists equal the folded pair's."""
import functools
import os

import numpy as np
import pytest
import torch

from foldh_model import (block_planes, buckets_of, entries_of, foldh_codes_of, max_entries, planted_holders, position_eh,
                         stream_planes)
from oracle import oracle
from poppunk_amd import engine, synth
from rank_fold2_model import fold2_codes_of, sorted_buckets
from rank_sort_model import order_of
from test_gpu_rank_fold2 import FOLD, FOLD2, RAW, jobs, last_kernel, make_db, run_jobs, tbl

pytestmark = pytest.mark.gpu

TOL = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")
KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
FOLDH = "dist_kernel_v2<256x32,lds-dma,rank 8,foldh>"
CASES = [(400, 16, 4), (400, 3, 4), (257, 8, 4), (400, 16, 64)]
# per k: (values with more than H holders, positions) planted over a spread of 0 .. 2
KEPT = {
    (400, 16, 4): [[(13, 3), (7, 1), (6, 60), (3, 70)], [(3, 10)], [], [(13, 70), (6, 200)], [(2, 100)]],
    (400, 3, 4): [[(14, 3), (7, 1), (6, 60), (3, 10)], [(3, 10)], [], [(13, 70)], [(6, 1)]],
    (257, 8, 4): [[(14, 3)], [(3, 10)], [(7, 100)], [], [(6, 64), (3, 64)]],
    (400, 16, 64): [[(3, 3), (2, 70)], [], [(3, 1)], [], []],
}


@functools.lru_cache(maxsize=None)
def planted(n, s64, h):
    """(sketches, bins, E_H per position)"""
    rng = np.random.default_rng(n + s64 + h)
    kept = rng.integers(0, 3 if h == 4 else 2, size=(len(KMERS), 64 * s64))
    for k, spec in enumerate(KEPT[n, s64, h]):
        free = list(rng.permutation(64 * s64))
        for value, count in spec:
            for _ in range(count):
                kept[k, free.pop()] = value
    bins = planted_holders(n, kept, h, seed=7 * n + s64 + h, folded=4 if h == 4 else 2)
    if (n, s64, h) == (400, 16, 4):
        bins[390] = bins[17]
    eh = position_eh(bins, h)
    assert block_planes(eh, order_of(eh)) is not None
    return synth.bitslice(bins, 14), bins, eh


def make_foldh_db(ppk_option, sk, s64, h, **kw):
    ppk_option("rank_foldh", 2)
    ppk_option("foldh_holders", h)
    ppk_option("foldh_min_planes", 2)
    return make_db(ppk_option, sk, s64, **kw)


@functools.lru_cache(maxsize=None)
def reference(n, s64, h):
    return {}


def raw_results(ppk_option, n, s64, h):
    """the raw planes' results, checked against the CPU oracle once per population"""
    ref = reference(n, s64, h)
    if not ref:
        sk = planted(n, s64, h)[0]
        db = make_foldh_db(ppk_option, sk, s64, h, rank=0)
        try:
            assert db.fold2_planes == 0 and db.foldh_holders() == 0
            ref.update(run_jobs(db, n))
            counts = engine.dist(db, None, KMERS, None, random_correct=False, counts=True)[0]
            assert np.array_equal(counts.cpu().numpy(), oracle.match_counts(sk, None, s64, 14, threads=4))
            want, wf = oracle.query(sk, None, KMERS, s64, 14, tbl(), threads=4)
            assert int(ref["whole"][1].item()) == wf
            assert np.abs(ref["whole"][0].cpu().numpy() - want).max() <= TOL
        finally:
            db.close()
        assert all(k == RAW for _, _, k in ref.values())
    return ref


def test_the_populations_reach_every_stream():
    for case in CASES:
        eh = planted(*case)[2]
        planes = block_planes(eh, order_of(eh))
        assert set(planes.ravel()) == ({2, 3, 4} if case[2] == 4 else {2, 3}), case
        assert (planes[:, 1:] <= planes[:, :-1]).all()
    eh = planted(400, 3, 4)[2]
    assert list(block_planes(eh, order_of(eh))[0]) == [4, 3, 2]
    assert {3, 4, 5, 8, 9, 16} <= set(eh.ravel())
    ent = entries_of(planted(400, 16, 4)[1], 4)
    twins = ent[(ent[:, 0] == 390) & (ent[:, 1] == 17)]      # (owed every bin whose value is not coded: far past 6 bits)
    assert len(twins) == 5 and (twins[:, 3] > 512).all() and ent[:, 3].max() == twins[:, 3].max() <= 1024


@pytest.mark.parametrize("n,s64,h", CASES)
def test_database_equals_the_model(ppk_option, n, s64, h):
    sk, bins, eh = planted(n, s64, h)
    db = make_foldh_db(ppk_option, sk, s64, h)
    try:
        order = order_of(eh)
        # (the duplicates share a thousand two-holder values: past the two-holder pair's 63 per (pair, k), which the
        # holder pair does not inherit -- that database keeps the folded pair beside it instead)
        twins = (n, s64, h) == (400, 16, 4)
        assert db.foldh_holders() == h and (db.fold2_planes, db.fold_planes) == ((0, 8) if twins else (8, 0))
        assert np.array_equal(db.foldh_position_order(), order)
        assert np.array_equal(db.foldh_stream_planes(), stream_planes(eh, order))
        for least in (3, 4):
            ppk_option("foldh_min_planes", least)
            assert np.array_equal(db.foldh_stream_planes(), stream_planes(eh, order, min_planes=least))
        ppk_option("foldh_min_planes", 2)
        ppk_option("rank_short", 0)
        assert (db.foldh_stream_planes() == 4).all()
        ppk_option("rank_short", 1)
        want_r, want_q = foldh_codes_of(bins, h)
        assert np.array_equal(db.foldh_codes(0), want_r) and np.array_equal(db.foldh_codes(1), want_q)
        ent = entries_of(bins, h)
        assert 0 < len(ent) <= max_entries(n, len(KMERS), 2)
        off, got = db.foldh_entries()
        want_off, want = buckets_of(ent, n)
        assert np.array_equal(off, want_off) and np.array_equal(sorted_buckets(off, got), want)
        # the two-holder pair beside it is what it was
        if not twins:
            want_r, want_q = fold2_codes_of(bins)
            assert np.array_equal(db.fold2_codes(0), want_r) and np.array_equal(db.fold2_codes(1), want_q)
    finally:
        db.close()


def test_the_default_rule_leaves_a_small_database_alone(ppk_option):
    """under four rounds of tiles: "rank_foldh" 1 builds nothing, 0 never does"""
    sk = planted(400, 3, 4)[0]
    for rule in (1, 0):
        ppk_option("rank_foldh", rule)
        ppk_option("foldh_holders", 4)
        db = make_db(ppk_option, sk, 3)
        try:
            assert db.foldh_holders() == 0 and db.fold2_planes == 8
            with pytest.raises(RuntimeError):
                db.foldh_entries()
            engine.dist(db, None, KMERS, tbl())
            torch.cuda.synchronize()
            assert last_kernel() == FOLD2
        finally:
            db.close()


@pytest.mark.parametrize("n,s64,h", CASES)
def test_same_bits_under_every_setting(ppk_option, n, s64, h):
    sk = planted(n, s64, h)[0]
    raw = raw_results(ppk_option, n, s64, h)
    db = make_foldh_db(ppk_option, sk, s64, h, fold2=0)
    try:
        assert db.fold2_planes == 0 and db.foldh_holders() == 0 and db.fold_planes == 8
        fold = run_jobs(db, n)
    finally:
        db.close()
    db = make_foldh_db(ppk_option, sk, s64, h)
    try:
        assert db.foldh_holders() == h
        got = run_jobs(db, n)
        ppk_option("foldh_min_planes", 3)
        three = run_jobs(db, n)
        ppk_option("foldh_min_planes", 4)
        four = run_jobs(db, n)
        ppk_option("foldh_min_planes", 2)
        ppk_option("rank_short", 0)
        full = run_jobs(db, n)
        ppk_option("rank_short", 1)
        ppk_option("rank_foldh", 0)          # at launch: the built pair is left unread
        fold2, beside = run_jobs(db, n), FOLD2 if db.fold2_planes else FOLD
    finally:
        db.close()
    for job, itself, _ in jobs(n):
        assert fold[job][2] == (RAW if itself else FOLD), job
        assert fold2[job][2] == (RAW if itself else beside), job
        for other in (got, three, four, full):
            assert other[job][2] == (RAW if itself else FOLDH), job
        for other in (three, four, full, fold2, fold, raw):
            assert torch.equal(got[job][0], other[job][0]) and torch.equal(got[job][1], other[job][1]), job


def test_fused_edge_lists(ppk_option):
    from poppunk_amd.models import BGMMModel
    n, s64, h = 400, 16, 4
    g = np.load(GOLDEN, allow_pickle=False)
    m = BGMMModel(g["k2_weights"], g["k2_means"], g["k2_covariances"], g["k2_scale"], g["k2_within"].item(),
                  g["k2_between"].item())
    sk = planted(n, s64, h)[0]
    dist = raw_results(ppk_option, n, s64, h)["whole"][0].cpu().numpy()
    x_max, y_max = synth.boundary_for_quantile(dist, 0.1)

    def lists(db, kernel):
        got = []
        for call in (lambda: engine.dist_edges(db, None, KMERS, tbl(), slope=2, x_max=x_max, y_max=y_max),
                     lambda: engine.dist_bgmm_edges(db, None, KMERS, tbl(), model=m.model)):
            edges, failed = call()
            torch.cuda.synchronize()
            assert last_kernel() == kernel
            got.append((edges.cpu().numpy(), int(failed.item())))
        return got

    db = make_foldh_db(ppk_option, sk, s64, h, fold2=0)
    try:
        ref = lists(db, FOLD)
    finally:
        db.close()
    assert 0 < len(ref[0][0]) < len(dist)
    db = make_foldh_db(ppk_option, sk, s64, h)
    try:
        got = lists(db, FOLDH)
    finally:
        db.close()
    for (ge, gf), (re_, rf) in zip(got, ref):
        assert np.array_equal(ge, re_) and gf == rf
