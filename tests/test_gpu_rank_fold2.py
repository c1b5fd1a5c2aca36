"""The two-holder pair of coded copies (PPK_CODING_FOLD2: the pair and its event list, option "rank_fold2"): every bin
value with exactly two holders is coded like a single-holder one, and the tile kernel adds the one match each is owed
back at the top of its epilogue.  n = 257 and n = 300: one full ref tile with its diagonal and half tiles and a strip.

The population is a related one three times over (every natural value has at least three holders), so every event is
planted -- or follows from a planting, which takes a holder away from a natural value; the model counts them all:
  (200, 10)             both holders in one tile
  (256, 40), (290, 270) the higher holder on the strip; both on the strip
  (250, 140)            a half tile (q >= r0 + 128)
  (100, 7), (101, 7)    refs 2l and 2l + 1 of one lane
  (60, 7), (188, 7)     refs 128 apart: registers r and r + 2 of one lane
  (222, 33)             three events at one k;  (223, 34): one at every k and two more at k 0
  (240, 150)            63 events at one k (the most a field holds); with one more the database keeps the folded pair
  (12, 77, 130)         a value with three holders stays coded
Checks: what the count pass found, the planes, the codes and the buckets equal tests/rank_fold2_model.py; the kernel is
the `,fold2` one; distances and n_failed are torch.equal to "rank_fold2" 0 (the folded pair) and to "rank_planes" 0
(the raw planes, whose counts and distances meet the CPU oracle) for the whole job, a band that cuts a tile and the
handle as its own query; the fused edge lists (line boundary and BGMM) equal those of "rank_fold2" 0."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from poppunk_amd import _lib, engine, synth
from rank_fold2_model import (MAX_PER_PAIR, SLOTS, block_counts, buckets_of, events_of, fold2_codes_of, per_pair_max,
                              sorted_buckets)
from rank_model import planes_of, unslice

pytestmark = pytest.mark.gpu

TOL = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")
KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
FOLD2 = "dist_kernel_v2<256x32,lds-dma,rank 8,fold2>"
FOLD = "dist_kernel_v2<256x32,lds-dma,rank 8,fold>"
RAW = "dist_kernel_v2<256x32,lds-dma>"


def last_kernel():
    return _lib.lib().ppk_last_kernel_name().decode()


@functools.lru_cache(maxsize=None)
def planted(n, s64=16, per_pair=MAX_PER_PAIR):
    """(sketches, bins, planted events): the tripled population with the plantings of the module docstring"""
    m = n // 3
    base = unslice(synth.make_sketches(m, KMERS, sketchsize64=s64, cluster_size=10)[0])
    base = np.where(base >= 16000, base - 8192, base).astype(np.uint16)      # (fresh values start at 16000)
    bins = np.concatenate([np.tile(base, (3, 1, 1)), base[:n - 3 * m]])
    fresh = iter(range(16000, 16384))
    want = []

    def event(hi, lo, k, pos):
        if hi >= n or lo >= n:
            return
        bins[[hi, lo], k, pos] = next(fresh)
        want.append((hi, lo, k))
    last = 64 * s64 - 1
    event(200, 10, 0, 0)
    event(256, 40, 1, last)
    event(290, 270, 1, 70)
    event(250, 140, 2, 65)
    event(100, 7, 3, 5)
    event(101, 7, 3, 6)
    event(60, 7, 4, 5)
    event(188, 7, 4, 6)
    for pos in (9, 200, last):
        event(222, 33, 2, pos)
    for k in range(5):
        event(223, 34, k, 300 + k)
    event(223, 34, 0, 310)
    event(223, 34, 0, 311)
    for pos in range(per_pair):
        event(240, 150, 4, 64 * 3 + pos)
    bins[[12, 77, 130], 0, 33] = next(fresh)
    got = set(map(tuple, events_of(bins)))
    assert set(want) <= got and len(got) > len(set(want))      # the plantings, and what they left of natural values
    assert per_pair_max(events_of(bins)) == per_pair
    return synth.bitslice(bins, 14), bins, want


@functools.lru_cache(maxsize=None)
def tbl():
    return synth.random_match_table(KMERS)


def make_db(ppk_option, sk, s64, rank=1, fold2=2):
    ppk_option("ksplit", 0)
    ppk_option("ksplit_long", 0)
    ppk_option("rank_planes", rank)
    ppk_option("rank_fold", 2)               # without the two-holder pair: the folded pair, gain or none
    ppk_option("rank_fold2", fold2)          # (the fixture restores it)
    ppk_option("rank_short", 1)
    return engine.SketchDB(sk, s64, 14)


def jobs(n):
    return [("whole", False, {}), ("band", False, dict(q_begin=37, q_end=n - 40)), ("itself", True, {})]


def run_jobs(db, n):
    out = {}
    for job, itself, band in jobs(n):
        d, failed = engine.dist(db, db if itself else None, KMERS, tbl(), **band)
        torch.cuda.synchronize()
        out[job] = (d.clone(), failed.clone(), last_kernel())
    return out


@functools.lru_cache(maxsize=None)
def reference(n, s64):
    """the raw planes' results of the planted population, checked against the CPU oracle once (set by the first test
    that needs them: the options are the fixture's)"""
    return {}


def raw_results(ppk_option, n, s64):
    ref = reference(n, s64)
    if not ref:
        sk = planted(n, s64)[0]
        db = make_db(ppk_option, sk, s64, rank=0)
        try:
            assert db.fold2_planes == 0 and db.rank_counts() is None
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


@pytest.mark.parametrize("n,s64", [(257, 16), (300, 16), (257, 8)])
def test_database_equals_the_model(ppk_option, n, s64):
    sk, bins, _ = planted(n, s64)
    bd, be, be2, two_max, two_total = block_counts(bins)
    p2, blocks2 = planes_of(be2)
    assert p2 == 8 and (blocks2 == 7).all() and two_max <= SLOTS
    db = make_db(ppk_option, sk, s64)
    try:
        c = db.rank_counts()
        assert (c["D"], c["E"], c["E2"]) == (bd.max(), be.max(), be2.max())
        assert np.array_equal(c["block_D"], bd) and np.array_equal(c["block_E"], be) and np.array_equal(c["block_E2"], be2)
        assert (c["two_max"], c["two_total"], c["pair_cap_hit"]) == (two_max, two_total, 0)
        assert db.fold2_planes == 8 and db.fold_planes == 0 and db.rank_planes == planes_of(bd)[0]
        assert np.array_equal(db.fold2_block_planes(), blocks2)
        want_r, want_q = fold2_codes_of(bins)
        assert np.array_equal(db.fold2_codes(0), want_r) and np.array_equal(db.fold2_codes(1), want_q)
        assert want_r[12, 0, 33] >= 2 and want_r[12, 0, 33] == want_r[77, 0, 33] == want_q[130, 0, 33]
        off, ev = db.fold2_events()
        want_off, want_ev = buckets_of(events_of(bins), n)
        assert np.array_equal(off, want_off) and np.array_equal(sorted_buckets(off, ev), want_ev)
    finally:
        db.close()


@pytest.mark.parametrize("n,s64", [(257, 16), (300, 16), (257, 8)])
def test_same_bits_as_the_folded_pair_and_the_raw_planes(ppk_option, n, s64):
    sk = planted(n, s64)[0]
    raw = raw_results(ppk_option, n, s64)
    db = make_db(ppk_option, sk, s64, fold2=0)
    try:
        assert db.fold2_planes == 0 and db.fold_planes == 8
        fold = run_jobs(db, n)
    finally:
        db.close()
    db = make_db(ppk_option, sk, s64)
    try:
        got = run_jobs(db, n)
        ppk_option("rank_fold2", 0)          # at launch: the built pair is left unread
        unread = run_jobs(db, n)
    finally:
        db.close()
    for job, itself, _ in jobs(n):
        assert fold[job][2] == (RAW if itself else FOLD) and got[job][2] == (RAW if itself else FOLD2), job
        assert unread[job][2] == RAW
        for other in (fold, raw, unread):
            assert torch.equal(got[job][0], other[job][0]) and torch.equal(got[job][1], other[job][1]), job


def test_one_event_too_many_keeps_the_folded_pair(ppk_option):
    n = 300
    sk, bins, _ = planted(n, 16, MAX_PER_PAIR + 1)
    db = make_db(ppk_option, sk, 16)
    try:
        c = db.rank_counts()
        assert c["pair_cap_hit"] == 1 and c["two_total"] == len(events_of(bins))
        assert db.fold2_planes == 0 and db.fold_planes == 8
        with pytest.raises(RuntimeError):
            db.fold2_events()
        got = run_jobs(db, n)
    finally:
        db.close()
    db = make_db(ppk_option, sk, 16, rank=0)
    try:
        want = run_jobs(db, n)
    finally:
        db.close()
    for job, itself, _ in jobs(n):
        assert got[job][2] == (RAW if itself else FOLD) and want[job][2] == RAW
        assert torch.equal(got[job][0], want[job][0]) and torch.equal(got[job][1], want[job][1])


def test_too_many_two_holder_values_at_a_position(ppk_option):
    """SLOTS + 1 two-holder values at one position of 530 genomes: the position cannot be listed, the pair is not built"""
    n = 530
    bins = unslice(synth.make_sketches(n, KMERS, cluster_size=10)[0])
    bins[:2 * (SLOTS + 1), 2, 100] = 16383 - np.arange(2 * (SLOTS + 1)) // 2
    bins[2 * (SLOTS + 1):, 2, 100] = 5
    two_max = block_counts(bins)[3]
    assert two_max >= SLOTS + 1
    db = make_db(ppk_option, synth.bitslice(bins, 14), 16)
    try:
        assert db.rank_counts()["two_max"] == two_max and db.fold2_planes == 0
    finally:
        db.close()


def test_default_leaves_a_small_database_its_folded_pair(ppk_option):
    sk = planted(300)[0]
    db = make_db(ppk_option, sk, 16, fold2=1)
    try:
        assert db.fold2_planes == 0 and db.fold_planes == 8
    finally:
        db.close()


@pytest.mark.parametrize("n", [257, 300])
def test_fused_edge_lists(ppk_option, n):
    from poppunk_amd.models import BGMMModel
    g = np.load(GOLDEN, allow_pickle=False)
    m = BGMMModel(g["k2_weights"], g["k2_means"], g["k2_covariances"], g["k2_scale"], g["k2_within"].item(),
                  g["k2_between"].item())
    sk = planted(n)[0]
    dist = raw_results(ppk_option, n, 16)["whole"][0].cpu().numpy()
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

    db = make_db(ppk_option, sk, 16, fold2=0)
    try:
        ref = lists(db, FOLD)
    finally:
        db.close()
    assert 0 < len(ref[0][0]) < len(dist)
    db = make_db(ppk_option, sk, 16)
    try:
        got = lists(db, FOLD2)
    finally:
        db.close()
    for (ge, gf), (re_, rf) in zip(got, ref):
        assert np.array_equal(ge, re_) and gf == rf
