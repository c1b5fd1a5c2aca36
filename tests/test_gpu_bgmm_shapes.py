"""GPU tests of BGMM assignment at every component count, alignment and row count its kernels branch on, against the
reference's own functions as recorded in tests/golden/bgmm_assign_k.npz (K = 1, 3, 5, 16, odd row counts) and
bgmm_assign.npz (K = 2, 4); tests/golden/make_golden_bgmm.py writes both.

Every expected label and responsibility is a recorded one: an input derived from a fixture case (a prefix, a cyclic
tiling, a view that starts one row later) is compared with the records of the same rows, never with a second device
call.  No row of these cases is undecided (tests/test_bgmm_host.py asserts it from the file), so labels are compared
exactly on every row, and responsibilities within 2 float32 ulp, as tests/test_gpu_bgmm.py does.

What each test reaches (ppk_launch_bgmm_assign, ppk_row_edges and kernel 1's epilogues choose by K and alignment):
  test_every_case_against_the_fixture        bgmm_assign_kernel<true, 0 | 3> with labels, values, both; ppk_bgmm_assign
  test_row_counts_alignments_and_sentinels   bgmm_assign_kernel<true | false, 0 | 2 | 3 | 4>, the one-row tail, NULL labels
  test_second_trip_of_the_grid_stride_loop   bgmm_assign_kernel<true | false, 3> past 2048 blocks x 2048 rows
  test_edge_lists_of_every_predicate         BgmmPred<3> and BgmmPred<0> counted (aligned), BgmmPred<0> uncounted (8-byte view)
  test_fused_paths                           the MODE_BGMM predicate of the LDS-table epilogue (k-split units, interior
                                             tiles), of the general epilogue (tile kernel, ragged tiles) and of the
                                             generic kernel, with K = 1, 3, 16; ppk_query_bgmm_edges_dbs with K = 3
(BgmmPred<2> and <4> counted: test_gpu_bgmm.py::test_edges_equal_generate_tuples_on_golden_labels.)"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from test_gpu_bgmm import case_model, fused_vs_two_step, synth_model, tuples, ulp_diff

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_CASES = ("k1", "k3", "k3_f64", "k5", "k16")
CASE_OF_K = {1: "k1", 2: "k2", 3: "k3", 4: "k4", 5: "k5", 16: "k16"}


@functools.lru_cache(maxsize=None)
def fixture_of(case):
    """The npz that holds `case` (loaded once; its arrays are read, never written)."""
    for name in ("bgmm_assign_k.npz", "bgmm_assign.npz"):
        g = np.load(os.path.join(HERE, "golden", name), allow_pickle=False)
        if case in list(g["cases"]):
            return {k: g[k] for k in g.files if k.startswith(case + "_")}
    raise KeyError(case)


def recorded(case, idx=None):
    """(model, X, labels, resp) of a case, or of its rows `idx`."""
    g = fixture_of(case)
    X, lab, resp = g[case + "_X"], g[case + "_labels"], g[case + "_resp"]
    if idx is not None:
        X, lab, resp = np.ascontiguousarray(X[idx]), lab[idx], resp[idx]
    return case_model(g, case), X, lab, resp


def with_within(case, within):
    """The case's model with another within label (ppk_bgmm_prepare stores it in the struct the predicates read)."""
    from poppunk_amd.models import BGMMModel
    g = fixture_of(case)
    return BGMMModel(g[case + "_weights"], g[case + "_means"], g[case + "_covariances"], g[case + "_scale"], within)


def first_rows(case, n):
    """Row indices of the first n rows of the case, the case repeated where it is shorter than n."""
    return np.arange(n) % fixture_of(case)[case + "_X"].shape[0]


@pytest.mark.parametrize("case", NEW_CASES)
def test_every_case_against_the_fixture(case):
    import torch
    from poppunk_amd import engine
    m, X, want, want_resp = recorded(case)
    K = m.n_components
    assert X.shape[0] % 2 == 1
    t = torch.from_numpy(X).cuda()
    lab, resp = engine.bgmm_assign_dev(t, m.model, True, True)
    lab_only, none = engine.bgmm_assign_dev(t, m.model, True, False)
    assert none is None
    none, resp_only = engine.bgmm_assign_dev(t, m.model, False, True)       # labels = NULL
    assert none is None
    lab, resp, lab_only, resp_only = (x.cpu().numpy() for x in (lab, resp, lab_only, resp_only))
    assert lab.dtype == np.int32 and resp.dtype == np.float32 and resp.shape == (X.shape[0], K)
    assert np.array_equal(lab, want)
    assert np.array_equal(lab_only, want)
    assert ulp_diff(resp, want_resp).max() <= 2
    assert np.array_equal(resp_only.view(np.uint32), resp.view(np.uint32))
    if K == 1:
        assert (lab == 0).all() and (resp == 1.0).all()
    # the host form, with the reference's dtypes
    y = m.assign(X)
    assert y.dtype == np.int64 and np.array_equal(y, want)
    r = m.assign(X, values=True)
    assert r.dtype == np.float32 and r.shape == (X.shape[0], K)
    assert ulp_diff(r, want_resp).max() <= 2
    assert np.array_equal(r.view(np.uint32), resp.view(np.uint32))


LAB_SENTINEL = -0x5a5a5a5b
RESP_SENTINEL = 0x7fc0beef          # (a NaN's bits: compared as integers)
PAD = 64                            # sentinel elements before and after each output


@pytest.mark.parametrize("K", sorted(CASE_OF_K))
def test_row_counts_alignments_and_sentinels(K):
    """One block's worth of rows (2048) and one more or less, and the smallest inputs, at the three placements that
    choose between the 16-byte and the 8-byte copy of the kernel.  The outputs lie inside larger buffers: what is
    written equals the fixture, and nothing before or after it is written at all."""
    import torch
    from poppunk_amd import _lib, engine
    case = CASE_OF_K[K]
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    stream = engine._stream_ptr(0)

    def run(in_t, n, lab_shift, want_labels=True):
        """Labels at element PAD + lab_shift of a sentinel-filled int32 buffer, responsibilities at element PAD of
        another; returns (labels, resp bits) after checking every sentinel."""
        lab_buf = torch.full((n + 2 * PAD,), LAB_SENTINEL, dtype=torch.int32, device=dev)
        resp_buf = torch.full((n * K + 2 * PAD,), RESP_SENTINEL, dtype=torch.int32, device=dev)
        lab_at = PAD + lab_shift
        lab_ptr = lab_buf.data_ptr() + 4 * lab_at
        resp_ptr = resp_buf.data_ptr() + 4 * PAD
        assert in_t.data_ptr() % 8 == 0 and resp_ptr % 4 == 0
        rc = lib.ppk_bgmm_assign_dev(C.c_void_p(in_t.data_ptr()), n, C.byref(m.model),
                                     C.c_void_p(lab_ptr) if want_labels else None, C.c_void_p(resp_ptr), stream)
        _lib.check(rc, "ppk_bgmm_assign_dev")
        torch.cuda.synchronize()
        lab_h, resp_h = lab_buf.cpu().numpy(), resp_buf.cpu().numpy()
        if want_labels:
            assert (lab_h[:lab_at] == LAB_SENTINEL).all() and (lab_h[lab_at + n:] == LAB_SENTINEL).all(), \
                "labels written outside [0, n)"
        else:
            assert (lab_h == LAB_SENTINEL).all()
        assert (resp_h[:PAD] == RESP_SENTINEL).all() and (resp_h[PAD + n * K:] == RESP_SENTINEL).all(), \
            "responsibilities written outside [0, n)"
        return lab_h[lab_at:lab_at + n], resp_h[PAD:PAD + n * K].view(np.float32).reshape(n, K)

    for n in (1, 2, 3, 1023, 2047, 2048, 2049):
        m, X, want, want_resp = recorded(case, first_rows(case, n))
        # rows 2.. of the buffer are 16-byte aligned, rows 1.. only 8-byte aligned
        in_buf = torch.zeros((n + 4, 2), dtype=torch.float32, device=dev)
        assert in_buf.data_ptr() % 16 == 0
        x = torch.from_numpy(X).to(dev)
        aligned_in, offset_in = in_buf[2:2 + n], in_buf[1:1 + n]
        assert aligned_in.data_ptr() % 16 == 0 and offset_in.data_ptr() % 16 == 8
        aligned_in.copy_(x)
        lab1, resp1 = run(aligned_in, n, 0)                 # 1: <true, KT>
        assert np.array_equal(lab1, want), (K, n, "aligned")
        assert ulp_diff(resp1, want_resp).max() <= 2, (K, n, "aligned")
        lab3, resp3 = run(aligned_in, n, 1)                 # 3: the labels pointer is 4 bytes off: <false, KT>
        assert np.array_equal(lab3, want) and np.array_equal(lab3, lab1), (K, n, "labels offset")
        assert ulp_diff(resp3, want_resp).max() <= 2, (K, n, "labels offset")
        in_buf.zero_()
        offset_in.copy_(x)
        lab2, resp2 = run(offset_in, n, 0)                  # 2: the input is 8 bytes off: <false, KT>
        assert np.array_equal(lab2, want) and np.array_equal(lab2, lab1), (K, n, "input offset")
        assert ulp_diff(resp2, want_resp).max() <= 2, (K, n, "input offset")
        _, resp_only = run(offset_in, n, 0, want_labels=False)
        assert np.array_equal(resp_only.view(np.uint32), resp2.view(np.uint32)), (K, n, "values only")


def test_second_trip_of_the_grid_stride_loop():
    """The grid is capped at 2048 blocks of 2048 rows: twice that and five rows more take the loop's second trip in
    every block and a third in the first.  The rows are k3's, repeated, so the recorded labels cover every one."""
    import torch
    from poppunk_amd import engine
    n = 2048 * 2048 * 2 + 5
    m, X, lab_case, resp_case = recorded("k3")
    rows = X.shape[0]
    idx = np.arange(n) % rows
    want = torch.from_numpy(lab_case.astype(np.int32)[idx]).cuda()
    tail = 4099
    want_resp = resp_case[idx[-tail:]]
    idx_t = torch.arange(n, device="cuda") % rows
    buf = torch.empty((n + 1, 2), dtype=torch.float32, device="cuda")
    buf[:n] = torch.from_numpy(X).cuda()[idx_t]
    for start in (0, 1):
        if start:
            buf[1:] = buf[:n].clone()
        t = buf[start:start + n]
        assert t.data_ptr() % 16 == 8 * start
        lab, resp = engine.bgmm_assign_dev(t, m.model, True, True)
        assert bool((lab == want).all()), "start %d: %d labels differ" % (start, int((lab != want).sum()))
        assert ulp_diff(resp[-tail:].cpu().numpy(), want_resp).max() <= 2, start
        del lab, resp


@pytest.mark.parametrize("K", (1, 3, 5, 16))
def test_edge_lists_of_every_predicate(K):
    """ppk_row_edges picks BgmmPred<3> or BgmmPred<0> with the counted mask on a 16-byte aligned matrix, and
    BgmmPred<0> with the row-order mask otherwise.  The rows are the case's, repeated to more than two compaction
    blocks of 16 384 rows; the expected list is generateTuples of the recorded labels of the same rows."""
    import torch
    from poppunk_amd import engine
    case = CASE_OF_K[K]
    own = int(fixture_of(case)[case + "_within"])
    n_ref = 37
    n_self = 259 * 258 // 2             # 33 411 rows: a condensed matrix of 259 samples
    n_rect = n_ref * 901                # 33 337 rows
    _, X, lab_all, _ = recorded(case, first_rows(case, n_self + 1))
    buf = torch.from_numpy(X).cuda()
    assert buf.data_ptr() % 16 == 0
    offset_given = False
    for within in sorted({0, K - 1, own}):
        m = with_within(case, within)
        for start in (0, 1):            # 0: aligned (counted mask); 1: an 8-byte aligned view (row-order mask)
            labels = lab_all[start:]
            t = buf[start:start + n_self]
            assert t.data_ptr() % 16 == 8 * start
            int_offset = 0 if offset_given or start == 0 else 7
            offset_given = offset_given or int_offset != 0
            cap = 100 if K == 1 else None       # K = 1: every row is an edge; too small a cap takes the exact re-run
            got = engine.bgmm_edges_dev(t, m.model, int_offset=int_offset, cap=cap).cpu().numpy()
            want = tuples(labels[:n_self], within, True, 0, int_offset)
            assert np.array_equal(got, want), (K, within, start, "self")
            if K == 1:
                assert got.shape[0] == n_self
            t = buf[start:start + n_rect]
            got = engine.bgmm_edges_dev(t, m.model, n_ref=n_ref, int_offset=11 * start, cap=cap).cpu().numpy()
            want = tuples(labels[:n_rect], within, False, n_ref, 11 * start)
            assert np.array_equal(got, want), (K, within, start, "n_ref")
            if K == 1:
                assert got.shape[0] == n_rect
    assert offset_given


def one_component(scale):
    from poppunk_amd.models import BGMMModel
    return BGMMModel([1.0], [[0.4, 0.5]], [[[0.05, 0.01], [0.01, 0.04]]], scale, 0, 0)


@pytest.mark.parametrize("K", (1, 3, 16))
def test_fused_paths(ppk_option, K):
    """Kernel 1's MODE_BGMM epilogues call ppk_bgmm_label with the run-time component loop.  The two-step side is
    ppk_bgmm_assign_dev, which the tests above tie to the reference, on the same distances: equal bit for bit."""
    from oracle import oracle
    from poppunk_amd import _lib, engine, synth

    def route(r, q, kl, tb, model):
        """the kernel a fused call of this job runs under the options set now"""
        engine.dist_bgmm_edges(r, q, kl, tb, model=model.model)
        return _lib.lib().ppk_last_kernel_name().decode()

    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n = 300
    sk, _ = synth.make_sketches(n, kmers, cluster_size=25)
    d, _ = oracle.query(sk[:120], None, kmers, 16, 14, tbl, threads=8)
    m = synth_model(d, K) if K > 1 else one_component(np.amax(d, axis=0))
    assert m.n_components == K
    all_pairs = n * (n - 1) // 2
    db = engine.SketchDB(sk, 16, 14, device=0)
    counts = [fused_vs_two_step(db, None, kmers, tbl, m)]                   # the default route (300 genomes: k-split units)
    assert "k-split" in route(db, None, kmers, tbl, m)
    ppk_option("ksplit", 1_000_000)                                         # forced on
    counts.append(fused_vs_two_step(db, None, kmers, tbl, m))
    assert "k-split" in route(db, None, kmers, tbl, m)
    ppk_option("ksplit", 0)                                                 # the tile kernel: ragged and diagonal tiles
    counts.append(fused_vs_two_step(db, None, kmers, tbl, m))
    assert "k-split" not in route(db, None, kmers, tbl, m)
    if K == 1:
        counts.append(fused_vs_two_step(db, None, kmers, tbl, m, cap=1000))     # short: the exact-size re-run
        assert counts == [all_pairs] * 4
    else:
        assert all(0 < c < all_pairs for c in counts), counts
    # reference x query under the tile kernel: 262 x 38 holds one interior tile (256 refs x 32 queries, LDS table)
    # and ragged ones (the general epilogue); then under the k-split
    ref = engine.SketchDB(sk[:262], 16, 14, device=0)
    qry = engine.SketchDB(sk[262:], 16, 14, device=0)
    got = fused_vs_two_step(ref, qry, kmers, tbl, m)
    assert "k-split" not in route(ref, qry, kmers, tbl, m)
    assert got == 262 * 38 if K == 1 else 0 < got < 262 * 38
    ppk_option("ksplit", 1_000_000)
    assert fused_vs_two_step(ref, qry, kmers, tbl, m) == got
    assert "k-split" in route(ref, qry, kmers, tbl, m)
    if K == 3:
        want, _ = m.edges_from_sketches(db, None, kmers, tbl)
        host, _ = m.edges_host(db, None, kmers, tbl)                        # ppk_query_bgmm_edges_dbs
        assert np.array_equal(host, want.cpu().numpy()) and host.shape[0] == counts[0]
    for x in (db, ref, qry):
        x.close()
    # a bbits = 16 database: the generic kernel's epilogue
    kk = np.asarray((13, 17, 21, 25, 29), dtype=np.int32)
    ksk, _ = synth.make_sketches(n, kk, bbits=16, cluster_size=25)
    ktbl = synth.random_match_table(kk)
    kdb = engine.SketchDB(ksk, 16, 16, device=0)
    kd, _ = engine.dist(kdb, None, kk, ktbl)
    kd = kd.cpu().numpy()[::7]
    m = synth_model(kd, K) if K > 1 else one_component(np.amax(kd, axis=0))
    ppk_option("ksplit", 0)
    got = fused_vs_two_step(kdb, None, kk, ktbl, m)
    assert "generic" in route(kdb, None, kk, ktbl, m)
    assert got == all_pairs if K == 1 else 0 < got < all_pairs
    kdb.close()
