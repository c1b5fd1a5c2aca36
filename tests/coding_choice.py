"""The choice among the coded copies as libppk_hip.so makes it (ppk_choose_coding, ppk_choose_holder: pure functions, no
device touched), next to the numpy models of tests/rank_fold2_model.py and tests/foldh_model.py.  `fold2_choice` and
`holder_choice` take what the models' `choice` take, ask both, assert that they agree and return the answer: every
assertion of tests/test_rank_fold2_host.py and tests/test_rank_foldh_host.py on the rule holds for the C++ as well."""
import ctypes as C

import numpy as np

import foldh_model
import rank_fold2_model
from poppunk_amd import _lib

NAMES = {2: "fold2", 1: "fold", 0: "rank", -1: "raw"}
SHORT_WORDS = 16


def counts_layout(bd, be, be2, two_max, two_total=0, pos_e2=None):
    """what the count pass reads back: the maxima of D, E, E2 over all positions and per block [nk, s64], the two-holder
    figures, E2 of every position [nk, 64 * s64] (default: every position as wide as its block)"""
    bd, be, be2 = (np.asarray(b, dtype=np.int64) for b in (bd, be, be2))
    if pos_e2 is None:
        pos_e2 = np.repeat(be2, 64, axis=1)
    assert pos_e2.shape == (bd.shape[0], 64 * bd.shape[1])
    parts = [np.concatenate([[b.max()], b.ravel()]) for b in (bd, be, be2)]
    return np.ascontiguousarray(np.concatenate(parts + [[two_max, two_total, 0], pos_e2.ravel()]), dtype=np.uint32)


def plan(counts, n, nk, s64, rank_fold=1, rank_fold2=1, fold2_sort=1, rank_foldh=1, tile_slots=512, bbits=14):
    """ppk_choose_coding: a dict of first, fallback (names), sums [3], order [nk, 64 * s64], seven / six [16] flag words,
    stream [nk, s64], stream_sum, try_holder"""
    first, fallback, try_holder, stream_sum = C.c_int(-9), C.c_int(-9), C.c_int(0), C.c_size_t(0)
    sums = (C.c_size_t * 3)()
    order = np.zeros((nk, 64 * s64), dtype=np.uint32)
    flags = np.zeros((2, SHORT_WORDS), dtype=np.uint32)
    stream = np.zeros((nk, s64), dtype=np.uint8)
    rc = _lib.lib().ppk_choose_coding(C.c_void_p(counts.ctypes.data), counts.size, n, nk, s64, bbits, tile_slots,
                                      (C.c_longlong * 4)(rank_fold, rank_fold2, fold2_sort, rank_foldh), C.byref(first),
                                      C.byref(fallback), sums, C.c_void_p(order.ctypes.data), C.c_void_p(flags.ctypes.data),
                                      C.c_void_p(stream.ctypes.data), C.byref(stream_sum), C.byref(try_holder))
    _lib.check(rc, "ppk_choose_coding")
    return {"first": NAMES[first.value], "fallback": NAMES[fallback.value], "sums": list(sums), "order": order,
            "seven": flags[0], "six": flags[1], "stream": stream, "stream_sum": stream_sum.value,
            "try_holder": bool(try_holder.value)}


def fold2_choice(bd, be, be2, two_max, pair_max, n, rank_fold=1, rank_fold2=1, tile_slots=512):
    """rank_fold2_model.choice and the library's answer, agreed.  The library learns of a (pair, k) past its event field
    only when it builds the pair: its answer is then the plan's fallback."""
    want = rank_fold2_model.choice(bd, be, be2, two_max, pair_max, n, rank_fold=rank_fold, rank_fold2=rank_fold2,
                                   tile_slots=tile_slots)
    nk, s64 = np.asarray(bd).shape
    p = plan(counts_layout(bd, be, be2, two_max), n, nk, s64, rank_fold=rank_fold, rank_fold2=rank_fold2,
             tile_slots=tile_slots)
    got = p["first"] if pair_max <= rank_fold2_model.MAX_PER_PAIR else p["fallback"]
    assert got == want, (got, want, p["first"], p["fallback"])
    sums = [rank_fold2_model.plane_sum(np.asarray(b))[0] for b in (bd, be, be2)]
    assert p["sums"] == sums, (p["sums"], sums)
    return want


def holder(eh_of, fold2_sum, n, nk, s64, rank_foldh=1, foldh_holders=0, tile_slots=512, most_shared=0):
    """ppk_choose_holder on E_H per position and rung (eh_of(h) -> [nk, 64 * s64]): (H or None, order [nk, 64 * s64],
    block planes [nk, s64], the cap on the entries)"""
    ladder = (foldh_holders,) + foldh_model.LADDER[1:] if foldh_holders else foldh_model.LADDER
    pos_e = np.ascontiguousarray(np.stack([np.asarray(eh_of(h)) for h in ladder], axis=-1), dtype=np.uint32)
    assert pos_e.shape == (nk, 64 * s64, len(foldh_model.LADDER))
    h, cap = C.c_uint(0), C.c_size_t(0)
    order = np.zeros((nk, 64 * s64), dtype=np.uint32)
    planes = np.zeros((nk, s64), dtype=np.uint8)
    rc = _lib.lib().ppk_choose_holder(C.c_void_p(pos_e.ctypes.data), pos_e.size, n, nk, s64, tile_slots, most_shared,
                                      fold2_sum, rank_foldh, foldh_holders, C.byref(h), C.c_void_p(order.ctypes.data),
                                      C.c_void_p(planes.ctypes.data), C.byref(cap))
    _lib.check(rc, "ppk_choose_holder")
    return (h.value or None), order, planes, cap.value


def holder_choice(eh_of, fold2_sum, n, nk, s64, rank_foldh=1, foldh_holders=0, tile_slots=512):
    """foldh_model.choice and the library's answer, agreed -- and with a pair, its order, block planes and cap"""
    want = foldh_model.choice(eh_of, fold2_sum, n, nk, s64, rank_foldh=rank_foldh, foldh_holders=foldh_holders,
                              tile_slots=tile_slots)
    got, order, planes, cap = holder(eh_of, fold2_sum, n, nk, s64, rank_foldh, foldh_holders, tile_slots)
    assert got == want, (got, want)
    if want is not None:
        eh = np.asarray(eh_of(want))
        assert np.array_equal(order, foldh_model.order_of(eh))
        assert np.array_equal(planes, foldh_model.block_planes(eh, order))
        assert cap == foldh_model.max_entries(n, nk, rank_foldh)
    return want
