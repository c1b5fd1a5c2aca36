"""The holder pair stored and copied as a 4-plane chunk (PPK_FOLDH_CHUNK_PLANES; tests/foldh_chunk_model.py): a block of
a tile is 8 ref pieces and one query piece, two DMA pieces per wavefront -- a ref piece each and wavefront 0's query
piece; in the half tile the odd wavefronts copy the ref pieces and wavefront 0 the query piece.

The planted populations of tests/test_gpu_rank_foldh.py (n = 400 at sketchsize64 16 and 3, n = 257 at 8, H forced to 4
and to 64).  Ref tile 0 of each has its four diagonal half tiles (queries 128 .. 255) and every population ends in a
strip; the band cuts both.  Checks, all exact:
  - ppk_db_foldh_read returns both copies word for word as the numpy statement gives them (padding samples included),
    asks for nk * sketchsize64 * 4 * npad words and refuses the 8-plane size;
  - distances and n_failed of the whole job and of a band, and both fused edge lists (line boundary and BGMM), under
    "foldh_min_planes" 2, 3 and 4 and "rank_short" 0 are those of "rank_foldh" 0 (the pair beside it) and of the raw
    planes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from foldh_chunk_model import CHUNK_PLANES, chunk_of
from foldh_model import foldh_codes_of
from poppunk_amd import _lib, engine, synth
from rank_sort_model import order_of
from test_gpu_rank_fold2 import FOLD, FOLD2, RAW, last_kernel, make_db, tbl
from test_gpu_rank_foldh import CASES, FOLDH, KMERS, make_foldh_db, planted

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")


def tiles_of(n, q_begin=0, q_end=None):
    """(half tiles, strip samples) a self job over query rows [q_begin, q_end) reaches: a diagonal half tile is a
    32-query tile of a whole 256-sample ref tile whose queries all lie beyond the tile's first 128 refs; the samples
    past the last whole ref tile are the strip"""
    q_end = n if q_end is None else q_end
    half = [(r0, q0) for r0 in range(0, n // 256 * 256, 256) for q0 in range(r0 + 128, r0 + 256, 32)
            if q0 + 32 > q_begin and q0 < q_end]
    return half, n % 256


def test_the_cases_reach_half_tiles_and_strips():
    for n, _, _ in CASES:
        for band in ({}, dict(q_begin=37, q_end=n - 40)):
            half, strip = tiles_of(n, **band)
            # (the band of n = 257 ends at row 217: it leaves the last of the four out)
            assert len(half) == (3 if band and n == 257 else 4) and strip > 0, (n, band)
    assert tiles_of(400)[1] == 144 and tiles_of(257)[1] == 1


@pytest.mark.parametrize("n,s64,h", CASES)
def test_both_copies_read_back_as_the_statement(ppk_option, n, s64, h):
    sk, bins, eh = planted(n, s64, h)
    order = order_of(eh)
    db = make_foldh_db(ppk_option, sk, s64, h)
    try:
        lib = _lib.lib()
        assert db.foldh_holders() == h and lib.ppk_db_foldh_chunk_planes(db._h) == CHUNK_PLANES
        npad = (n + 255) // 256 * 256
        for which, want in enumerate(foldh_codes_of(bins, h)):
            raw = np.full((len(KMERS), s64, CHUNK_PLANES, npad), np.uint64(0x5555555555555555), dtype=np.uint64)
            _lib.check(lib.ppk_db_foldh_read(db._h, which, C.c_void_p(raw.ctypes.data), raw.size), "ppk_db_foldh_read")
            assert np.array_equal(raw, chunk_of(want, order)), which
            assert np.array_equal(db.foldh_codes(which), want)
        eight = np.zeros(2 * raw.size, dtype=np.uint64)
        assert lib.ppk_db_foldh_read(db._h, 0, C.c_void_p(eight.ctypes.data), eight.size) == _lib.ERR_ARG
        assert not eight.any()
    finally:
        db.close()
    # without the pair: no chunk
    db = make_db(ppk_option, sk, s64, rank=0)
    try:
        assert _lib.lib().ppk_db_foldh_chunk_planes(db._h) == 0
    finally:
        db.close()


def bgmm_model():
    from poppunk_amd.models import BGMMModel
    g = np.load(GOLDEN, allow_pickle=False)
    return BGMMModel(g["k2_weights"], g["k2_means"], g["k2_covariances"], g["k2_scale"], g["k2_within"].item(),
                     g["k2_between"].item()).model


def run_all(db, n, boundary, kernel):
    """whole job, band and both fused edge lists; every launch is `kernel`"""
    out = {}
    for job, band in (("whole", {}), ("band", dict(q_begin=37, q_end=n - 40))):
        d, failed = engine.dist(db, None, KMERS, tbl(), **band)
        torch.cuda.synchronize()
        assert last_kernel() == kernel, (job, last_kernel())
        out[job] = (d.clone(), failed.clone())
    if boundary is None:
        boundary = synth.boundary_for_quantile(out["whole"][0].cpu().numpy(), 0.1)
    x_max, y_max = boundary
    for job, call in (("line", lambda: engine.dist_edges(db, None, KMERS, tbl(), slope=2, x_max=x_max, y_max=y_max)),
                      ("bgmm", lambda: engine.dist_bgmm_edges(db, None, KMERS, tbl(), model=bgmm_model()))):
        edges, failed = call()
        torch.cuda.synchronize()
        assert last_kernel() == kernel, (job, last_kernel())
        out[job] = (edges.clone(), failed.clone())
    return out, boundary


@pytest.mark.parametrize("n,s64,h", CASES)
def test_same_bits_whole_band_and_edge_lists(ppk_option, n, s64, h):
    sk = planted(n, s64, h)[0]
    db = make_foldh_db(ppk_option, sk, s64, h, rank=0)
    try:
        assert db.foldh_holders() == 0
        raw, boundary = run_all(db, n, None, RAW)
    finally:
        db.close()
    assert 0 < len(raw["line"][0]) < len(raw["whole"][0])
    db = make_foldh_db(ppk_option, sk, s64, h)
    try:
        assert db.foldh_holders() == h
        got = {}
        for least in (2, 3, 4):
            ppk_option("foldh_min_planes", least)
            got["min_planes %d" % least] = run_all(db, n, boundary, FOLDH)[0]
        ppk_option("foldh_min_planes", 2)
        ppk_option("rank_short", 0)
        got["rank_short 0"] = run_all(db, n, boundary, FOLDH)[0]
        ppk_option("rank_short", 1)
        ppk_option("rank_foldh", 0)          # at launch: the pair beside it
        beside = run_all(db, n, boundary, FOLD2 if db.fold2_planes else FOLD)[0]
    finally:
        db.close()
    for setting, res in got.items():
        for job in ("whole", "band", "line", "bgmm"):
            for other in (beside, raw):
                assert torch.equal(res[job][0], other[job][0]) and torch.equal(res[job][1], other[job][1]), (setting, job)
