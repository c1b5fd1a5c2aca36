"""The two-holder pair with its positions sorted by code span (options "fold2_sort", "fold2_min_planes"): slot i of k
holds stored position fold2_position_order()[k, i], and a block of slots compares 8, 7 or 6 planes by its widest E2.

Populations are planted to a chosen E2 per position (tests/rank_sort_model.py: E2 - 2 values with three holders or more,
exactly three at the widest positions, a few two-holder values -- the events -- and every other sample a value of its
own):
  n = 400, sketchsize64 16 and 3: positions at E2 = 64, 65, 128 and 129 over a spread of 20 .. 64, a different mix per k
                                  (one k without a position above 128, one without any above 64); at sketchsize64 3 the
                                  three blocks of k 0 compare 8, 7 and 6 planes
  n = 257, sketchsize64 8:        the second ref tile holds one sample; at most 83 values with three holders, so 7
                                  and 6 planes only
Checks: the device's order and stream planes equal the model under every setting of the options; the codes in stored
order, the per-block figures and the events are what they were; distances and n_failed are torch.equal for the whole
job, a band that cuts a tile and the handle as its own query against "fold2_sort" 0, "fold2_min_planes" 7, "rank_short"
0, "rank_fold2" 0 (the folded pair) and "rank_planes" 0 (the raw planes, whose counts and distances meet the CPU
oracle); both fused edge lists equal the folded pair's."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from poppunk_amd import engine, synth
from rank_fold2_model import (MAX_PER_PAIR, SLOTS, block_counts, buckets_of, events_of, fold2_codes_of, per_pair_max,
                              sorted_buckets)
from rank_model import planes_of
from rank_sort_model import order_of, planted_e2, position_e2, spread_targets, stream_planes
from test_gpu_rank_fold2 import FOLD, FOLD2, RAW, jobs, last_kernel, make_db, run_jobs, tbl

pytestmark = pytest.mark.gpu

TOL = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")
KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
CASES = [(400, 16), (400, 3), (257, 8)]
# per k: (E2, positions) planted over the spread
WIDE = {
    (400, 16): [[(129, 3), (133, 1), (128, 2), (65, 70), (64, 5)], [(128, 1), (65, 1), (100, 130), (64, 9)], [(64, 40)],
                [(129, 65), (128, 64), (65, 64)], [(65, 1)]],
    (400, 3): [[(129, 2), (128, 3), (65, 70), (64, 4)], [(128, 64), (65, 1)], [(64, 3)], [(129, 1)], [(65, 128)]],
    (257, 8): [[(85, 3), (65, 70), (64, 4)], [(65, 1)], [(64, 64)], [(80, 64), (66, 64)], []],
}


@functools.lru_cache(maxsize=None)
def planted(n, s64):
    """(sketches, bins, E2 per position)"""
    targets = spread_targets(len(KMERS), 64 * s64, 133 if n == 400 else 85, seed=n + s64, wide=WIDE[n, s64])
    bins = planted_e2(n, targets, seed=7 * n + s64)
    e2 = position_e2(bins)
    assert np.array_equal(e2, targets) and 0 < per_pair_max(events_of(bins)) <= MAX_PER_PAIR
    return synth.bitslice(bins, 14), bins, e2


@functools.lru_cache(maxsize=None)
def reference(n, s64):
    return {}


def raw_results(ppk_option, n, s64):
    """the raw planes' results, checked against the CPU oracle once per population"""
    ref = reference(n, s64)
    if not ref:
        sk = planted(n, s64)[0]
        db = make_db(ppk_option, sk, s64, rank=0)
        try:
            assert db.fold2_planes == 0
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
    for (n, s64) in CASES:
        e2 = planted(n, s64)[2]
        planes = stream_planes(e2, order_of(e2))
        assert set(planes.ravel()) == ({6, 7, 8} if n == 400 else {6, 7})
        assert (planes[:, 1:] <= planes[:, :-1]).all()
        assert planes.sum() < stream_planes(e2, order_of(e2, sort=False)).sum()
    e2 = planted(400, 3)[2]
    assert list(stream_planes(e2, order_of(e2))[0]) == [8, 7, 6]
    assert {64, 65, 128, 129} <= set(planted(400, 16)[2].ravel()) and {64, 65, 128, 129} <= set(e2.ravel())


@pytest.mark.parametrize("n,s64", CASES)
def test_database_equals_the_model(ppk_option, n, s64):
    sk, bins, e2 = planted(n, s64)
    bd, be, be2, two_max, two_total = block_counts(bins)
    assert two_max <= SLOTS and two_total > 0
    for sort in (1, 0):
        ppk_option("fold2_sort", sort)
        ppk_option("fold2_min_planes", 6)
        db = make_db(ppk_option, sk, s64)
        try:
            order = order_of(e2, sort=bool(sort))
            assert db.fold2_planes == 8 and db.fold_planes == 0
            assert np.array_equal(db.fold2_position_order(), order)
            assert np.array_equal(db.fold2_stream_planes(), stream_planes(e2, order))
            ppk_option("fold2_min_planes", 7)
            assert np.array_equal(db.fold2_stream_planes(), stream_planes(e2, order, min_planes=7))
            ppk_option("fold2_min_planes", 6)
            ppk_option("rank_short", 0)
            assert (db.fold2_stream_planes() == 8).all()
            ppk_option("rank_short", 1)
            # what existing callers read keeps its meaning: stored blocks, stored position order
            c = db.rank_counts()
            assert np.array_equal(c["block_E2"], be2)
            assert (c["two_max"], c["two_total"], c["pair_cap_hit"]) == (two_max, two_total, 0)
            assert np.array_equal(db.fold2_block_planes(), planes_of(be2)[1])
            want_r, want_q = fold2_codes_of(bins)
            assert np.array_equal(db.fold2_codes(0), want_r) and np.array_equal(db.fold2_codes(1), want_q)
            off, ev = db.fold2_events()
            want_off, want_ev = buckets_of(events_of(bins), n)
            assert np.array_equal(off, want_off) and np.array_equal(sorted_buckets(off, ev), want_ev)
        finally:
            db.close()


@pytest.mark.parametrize("n,s64", CASES)
def test_same_bits_under_every_setting(ppk_option, n, s64):
    sk = planted(n, s64)[0]
    raw = raw_results(ppk_option, n, s64)
    ppk_option("fold2_sort", 1)
    ppk_option("fold2_min_planes", 6)
    db = make_db(ppk_option, sk, s64, fold2=0)
    try:
        assert db.fold2_planes == 0 and db.fold_planes == 8
        fold = run_jobs(db, n)
    finally:
        db.close()
    ppk_option("fold2_sort", 0)
    db = make_db(ppk_option, sk, s64)
    try:
        unsorted = run_jobs(db, n)
    finally:
        db.close()
    ppk_option("fold2_sort", 1)
    db = make_db(ppk_option, sk, s64)
    try:
        got = run_jobs(db, n)
        ppk_option("fold2_min_planes", 7)
        seven = run_jobs(db, n)
        ppk_option("fold2_min_planes", 6)
        ppk_option("rank_short", 0)
        full = run_jobs(db, n)
        ppk_option("rank_short", 1)
    finally:
        db.close()
    for job, itself, _ in jobs(n):
        assert fold[job][2] == (RAW if itself else FOLD), job
        for other in (got, unsorted, seven, full):
            assert other[job][2] == (RAW if itself else FOLD2), job
        for other in (unsorted, seven, full, fold, raw):
            assert torch.equal(got[job][0], other[job][0]) and torch.equal(got[job][1], other[job][1]), job


def test_fused_edge_lists(ppk_option):
    from poppunk_amd.models import BGMMModel
    n, s64 = 400, 16
    g = np.load(GOLDEN, allow_pickle=False)
    m = BGMMModel(g["k2_weights"], g["k2_means"], g["k2_covariances"], g["k2_scale"], g["k2_within"].item(),
                  g["k2_between"].item())
    sk = planted(n, s64)[0]
    dist = raw_results(ppk_option, n, s64)["whole"][0].cpu().numpy()
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

    ppk_option("fold2_sort", 1)
    ppk_option("fold2_min_planes", 6)
    db = make_db(ppk_option, sk, s64, fold2=0)
    try:
        ref = lists(db, FOLD)
    finally:
        db.close()
    assert 0 < len(ref[0][0]) < len(dist)
    db = make_db(ppk_option, sk, s64)
    try:
        got = lists(db, FOLD2)
    finally:
        db.close()
    for (ge, gf), (re_, rf) in zip(got, ref):
        assert np.array_equal(ge, re_) and gf == rf
