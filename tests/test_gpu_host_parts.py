"""The device-list frame of the host query calls (ppk_host.hip) on a real MI355X: a device list becomes entries,
every entry takes a band of query rows, and the entries' results are put together.  Dense distances, fused edge lists
and neighbour lists at the smallest sizes at which an entry's band is empty, one tile, or straddles a 64-query band
edge of ppk_band_split: the multi-entry result equals the one-entry result bit for bit, the one-entry result agrees
with the CPU oracle, and every argument error leaves the next correct call untouched.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from oracle import oracle
from poppunk_amd import _lib, engine, poppunk_refine, pp_sketchlib, synth
from test_gpu_bgmm import synth_model

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
TOL = 1e-6
LISTS = [(0,), (0, 0), (0, 0, 0, 0)]
SELF_N = (1, 2, 65, 130)
REF_QRY = ((70, 1), (70, 129))
SHAPES = [(n, 0) for n in SELF_N] + list(REF_QRY)


@functools.lru_cache(maxsize=None)
def _table():
    return synth.random_match_table(KMERS)


@functools.lru_cache(maxsize=None)
def _job(n_ref, n_qry):
    """(ref sketches, query sketches or None, the one-entry distances, a boundary with about a third of the pairs
    inside).  Computed once per shape; the arrays are read, never written."""
    sk, _ = synth.make_sketches(n_ref + n_qry, KMERS, cluster_size=13, seed=1000 + 7 * n_ref + n_qry)
    ref, qry = (sk[:n_ref], sk[n_ref:]) if n_qry else (sk, None)
    dist, n_failed = pp_sketchlib.query_arrays(ref, qry, KMERS, 16, 14, _table(), devices=(0,))
    assert n_failed == 0
    x_max, y_max = synth.boundary_for_quantile(dist, 0.17) if len(dist) else (0.1, 0.1)
    return ref, qry, dist, (x_max, y_max)


def _stats():
    v = (C.c_double * 8)()
    _lib.check(_lib.lib().ppk_query_last_stats(v, 8), "ppk_query_last_stats")
    return {"parts": v[0], "threads": v[1]}


# ---- dense distances -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ref,n_qry", SHAPES)
def test_dense_distances_over_device_lists(n_ref, n_qry):
    ref, qry, base, _ = _job(n_ref, n_qry)
    assert base.shape == ((n_ref * n_qry if n_qry else n_ref * (n_ref - 1) // 2), 2)      # n = 1: an empty array
    if len(base):
        want, failed = oracle.query(ref, qry, KMERS, 16, 14, _table(), threads=4)
        assert failed == 0 and np.abs(base - want).max() <= TOL
    for devices in LISTS[1:]:
        got, n_failed = pp_sketchlib.query_arrays(ref, qry, KMERS, 16, 14, _table(), devices=devices)
        assert n_failed == 0 and np.array_equal(got, base), devices
    # the resident-handle form: a list of handles is the device list
    rdb = engine.SketchDB(ref, 16, 14)
    qdb = engine.SketchDB(qry, 16, 14) if n_qry else None
    for devices in LISTS:
        rc, got = _dense_dbs([rdb._h.value] * len(devices), [qdb._h.value] * len(devices) if qdb else None, len(base))
        assert rc == _lib.OK and np.array_equal(got, base), devices
    rdb.close()
    if qdb:
        qdb.close()


def test_dense_stats_count_entries_and_threads():
    ref, _, base, _ = _job(130, 0)
    got, _ = pp_sketchlib.query_arrays(ref, None, KMERS, 16, 14, _table(), devices=(0, 0))
    assert np.array_equal(got, base) and _stats() == {"parts": 2, "threads": 2}
    got, _ = pp_sketchlib.query_arrays(ref, None, KMERS, 16, 14, _table(), devices=(0,))
    assert np.array_equal(got, base) and _stats() == {"parts": 1, "threads": 0}


# ---- fused edge lists ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ref,n_qry", SHAPES)
def test_edge_lists_over_device_lists(n_ref, n_qry):
    ref, qry, dist, (x_max, y_max) = _job(n_ref, n_qry)

    def edges(devices, **kw):
        got, n_failed = pp_sketchlib.query_edges_arrays(ref, qry, KMERS, 16, 14, 2, x_max, y_max, random_table=_table(),
                                                        devices=devices, **kw)
        assert n_failed == 0 and got.dtype == np.int64
        return got

    base = edges((0,))
    if len(dist):
        want = oracle.edge_threshold(dist, 2, x_max, y_max, n_ref=n_ref if n_qry else 0, inclusive=True)
        assert np.array_equal(base, want)
        assert 0 < len(want) < max(len(dist), 2)
    else:
        assert base.shape == (0, 2)                                   # n = 1: an empty list
    for devices in LISTS[1:]:
        assert np.array_equal(edges(devices), base), devices
    # cap below the count: the finished multi-entry list is parked on the host and fetched
    for devices in LISTS:
        assert np.array_equal(edges(devices, cap=0), base), devices
    # the handle form reaches the library at n = 1 too (the array form answers an empty job itself)
    rdb = engine.SketchDB(ref, 16, 14)
    qdb = engine.SketchDB(qry, 16, 14) if n_qry else None
    for devices in LISTS:
        got, _ = engine.edges_host([rdb] * len(devices), [qdb] * len(devices) if qdb else None, KMERS, _table(),
                                   slope=2, x_max=x_max, y_max=y_max)
        assert np.array_equal(got, base), devices
    rdb.close()
    if qdb:
        qdb.close()


def test_bgmm_edge_lists_over_device_lists():
    ref, _, dist, _ = _job(130, 0)
    m = synth_model(dist, 2)
    db = engine.SketchDB(ref, 16, 14)
    want, _ = m.edges_from_sketches(db, None, KMERS, _table())
    want = want.cpu().numpy()
    assert 0 < len(want) < len(dist)
    for devices in LISTS:
        got, _ = m.edges_host([db] * len(devices), None, KMERS, _table())
        assert np.array_equal(got, want), devices
        got, _ = m.edges_host([db] * len(devices), None, KMERS, _table(), cap=1)
        assert np.array_equal(got, want), devices
    db.close()


# ---- neighbour lists -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SELF_N)
def test_neighbour_lists_over_device_lists(n):
    sk, _, dist, _ = _job(n, 0)
    for knn, col in ((3, 0), (6, 1)):
        base = pp_sketchlib.query_knn_arrays(sk, KMERS, 16, 14, knn, col, _table(), devices=(0,))
        if n == 1:                                                    # no other sample: (i, 0, 0.0) in every slot
            want = (np.zeros(knn, np.int64), np.zeros(knn, np.int64), np.zeros(knn, np.float32))
        else:
            want = oracle.knn(oracle.long_to_square(dist[:, col]), knn)
        for g, w in zip(base, want):
            assert np.array_equal(g, w), (knn, col)
        for devices in LISTS[1:]:
            got = pp_sketchlib.query_knn_arrays(sk, KMERS, 16, 14, knn, col, _table(), devices=devices)
            for g, b in zip(got, base):
                assert np.array_equal(g, b), (devices, knn, col)


def test_extend_from_sketches_over_device_lists():
    n_ref, n_qry = 70, 129
    ref, qry, qr, _ = _job(n_ref, n_qry)
    rr, _ = pp_sketchlib.query_arrays(ref, None, KMERS, 16, 14, _table())
    qq, _ = pp_sketchlib.query_arrays(qry, None, KMERS, 16, 14, _table())
    rdb, qdb = engine.SketchDB(ref, 16, 14), engine.SketchDB(qry, 16, 14)
    for col, knn in ((0, 5), (1, 3)):
        coo = oracle.knn(oracle.long_to_square(rr[:, col]), knn)
        qq_sq = oracle.long_to_square(qq[:, col])
        qr_rect = np.ascontiguousarray(qr[:, col].reshape(n_qry, n_ref).T)
        want = poppunk_refine.extend_arrays(coo, qq_sq, qr_rect, knn)
        for devices in ((0,), (0, 0, 0, 0)):
            got = engine.extend_from_sketches(coo, [rdb] * len(devices), [qdb] * len(devices), KMERS, _table(), knn,
                                              dist_col=col)
            for g, w in zip(got, want):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (devices, col)
    rdb.close()
    qdb.close()


# ---- argument errors: every family, one table ----------------------------------------------------------------------

def _handles(h):
    return (C.c_void_p * len(h))(*h) if h is not None else None


def _kp():
    return KMERS.ctypes.data_as(C.POINTER(C.c_int32))


def _tp():
    return _table().ctypes.data_as(C.POINTER(C.c_float))


FLAGS = _lib.FLAG_RANDOM_CORRECT
LLP = C.POINTER(C.c_longlong)


def _dense_dbs(refs, qrys, rows):
    out = np.zeros((max(rows, 1), 2), dtype=np.float32)
    rc = _lib.lib().ppk_query_dbs(_handles(refs), _handles(qrys), len(refs), _kp(), _tp(), 1, FLAGS,
                                  C.c_void_p(out.ctypes.data), None)
    return rc, out[:rows]


def _edges_dbs(refs, qrys, model=None):
    out = np.zeros((1 << 15, 2), dtype=np.int64)
    n = C.c_size_t(0)
    lib = _lib.lib()
    if model is None:
        rc = lib.ppk_query_edges_dbs(_handles(refs), _handles(qrys), len(refs), _kp(), _tp(), 1, FLAGS, 2, 0.05, 0.05,
                                     1.0, 1.0, 1, out.ctypes.data_as(LLP), len(out), C.byref(n), None)
    else:
        rc = lib.ppk_query_bgmm_edges_dbs(_handles(refs), _handles(qrys), len(refs), _kp(), _tp(), 1, FLAGS,
                                          C.byref(model), out.ctypes.data_as(LLP), len(out), C.byref(n), None)
    return rc, out[:n.value]


def _knn_dbs(dbs, n):
    oi, oj, od = np.zeros(n * 3, np.int64), np.zeros(n * 3, np.int64), np.zeros(n * 3, np.float32)
    rc = _lib.lib().ppk_query_knn_dbs(_handles(dbs), len(dbs), _kp(), _tp(), 1, FLAGS, 3, 0, oi.ctypes.data_as(LLP),
                                      oj.ctypes.data_as(LLP), od.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, np.concatenate([oi, oj, od.view(np.int32)])


def _extend_dbs(refs, qrys, n_all):
    cap = n_all * 3
    oi, oj, od = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.float32)
    n = C.c_size_t(0)
    rc = _lib.lib().ppk_extend_sketches_dbs(None, None, None, 0, _handles(refs), _handles(qrys), len(refs), _kp(), _tp(),
                                            1, FLAGS, 3, 0, oi.ctypes.data_as(LLP), oj.ctypes.data_as(LLP),
                                            od.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n))
    return rc, np.concatenate([oi[:n.value], oj[:n.value], od[:n.value].view(np.int32)])


def test_argument_errors_of_every_family_leave_the_next_call_untouched():
    """A device listed five times, per-device handles of different n, a missing handle, ref and query handles with
    different k-mer lists, a device id out of range: PPK_ERR_ARG from every family, and the same thread's next correct
    call gives the baseline bit for bit.  Only arguments are wrong: nothing here reaches a kernel."""
    ref, qry, _, _ = _job(70, 129)
    a = engine.SketchDB(ref, 16, 14)
    b = engine.SketchDB(ref[:65], 16, 14)                                          # another n
    q = engine.SketchDB(qry, 16, 14)
    q4 = engine.SketchDB(np.ascontiguousarray(qry[:, :4]), 16, 14)                  # four k-mer lengths, not five
    ha, hb, hq, hq4 = (x._h.value for x in (a, b, q, q4))
    model = synth_model(_job(130, 0)[2], 2).model
    n_all = 70 + 129
    families = {
        "dense": lambda r, qs: _dense_dbs(r, qs, 70 * 129 if qs else 70 * 69 // 2),
        "edges": lambda r, qs: _edges_dbs(r, qs),
        "bgmm edges": lambda r, qs: _edges_dbs(r, qs, model),
        "knn": lambda r, qs: _extend_dbs(r, qs, n_all) if qs else _knn_dbs(r, 70),
    }
    bad = {
        "five times": ([ha] * 5, None, "at most 4"),
        "different n": ([ha, hb], None, None),
        "missing handle": ([ha, None], None, None),
        "k-mer lists": ([ha], [hq4], None),
    }
    for fam, call in families.items():
        base_self = call([ha], None)
        base_rq = call([ha], [hq])
        assert base_self[0] == _lib.OK and base_rq[0] == _lib.OK, fam
        for what, (refs, qrys, message) in bad.items():
            rc, _ = call(refs, qrys)
            assert rc == _lib.ERR_ARG, (fam, what, _lib.last_error())
            if message:
                assert message in _lib.last_error(), (fam, what)
            again = call([ha], [hq]) if qrys else call([ha], None)
            want = base_rq if qrys else base_self
            assert again[0] == _lib.OK and np.array_equal(again[1], want[1]), (fam, what)
    for x in (a, b, q, q4):
        x.close()
    # the host-array entries take the device list itself
    sk, _, dist, (x_max, y_max) = _job(130, 0)
    arrays = {
        "dense": lambda d: pp_sketchlib.query_arrays(sk, None, KMERS, 16, 14, _table(), devices=d)[0],
        "edges": lambda d: pp_sketchlib.query_edges_arrays(sk, None, KMERS, 16, 14, 2, x_max, y_max,
                                                           random_table=_table(), devices=d)[0],
        "knn": lambda d: np.concatenate([np.asarray(x).view(np.int32) if x.dtype == np.float32 else x for x in
                                         pp_sketchlib.query_knn_arrays(sk, KMERS, 16, 14, 3, 0, _table(), devices=d)]),
    }
    arg_error = re.escape("failed (%d)" % _lib.ERR_ARG)
    for fam, call in arrays.items():
        base = call((0,))
        for devices, message in (((0,) * 5, "at most 4"), ((-1,), arg_error), ((0, 1 << 20), arg_error)):
            with pytest.raises(RuntimeError, match=message) as err:
                call(devices)
            assert re.search(arg_error, str(err.value)), (fam, devices)
            assert np.array_equal(call((0,)), base), (fam, devices)
    pp_sketchlib.clear_cache()
