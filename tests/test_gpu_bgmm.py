"""GPU tests of BGMM assignment: kernel 2 against the reference-derived golden (tests/golden/bgmm_assign.npz), the
edge lists against generateTuples, and the fused sketches -> BGMM -> edge list path against the two-step one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgmm_assign.npz")
SKLEARN_FITS = ("k2", "k2_f64", "k4")


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def case_model(g, case):
    from poppunk_amd.models import BGMMModel
    return BGMMModel(g[case + "_weights"], g[case + "_means"], g[case + "_covariances"], g[case + "_scale"],
                     g[case + "_within"].item(), g[case + "_between"].item())


def tuples(labels, within, self_comparison, num_ref=0, int_offset=0):
    from oracle import oracle
    return oracle.generate_tuples(np.asarray(labels, dtype=np.int32), within, self_comparison, num_ref, int_offset)


def ulp_diff(a, b):
    a = a.astype(np.float32).view(np.int32).astype(np.int64)
    b = b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_labels_and_responsibilities_match_golden():
    import torch
    g = golden()
    for case in list(g["cases"]):
        m = case_model(g, case)
        X = g[case + "_X"]
        t = torch.from_numpy(X).cuda()
        lab, resp = __import__("poppunk_amd.engine", fromlist=["x"]).bgmm_assign_dev(t, m.model, True, True)
        lab, resp = lab.cpu().numpy(), resp.cpu().numpy()
        lab_only, _ = __import__("poppunk_amd.engine", fromlist=["x"]).bgmm_assign_dev(t, m.model, True, False)
        assert np.array_equal(lab_only.cpu().numpy(), lab), case
        want = g[case + "_labels"]
        decided = g[case + "_gap"] > 1e-9 * np.maximum(1.0, np.abs(g[case + "_top"]))
        if case in SKLEARN_FITS:
            assert decided.all(), "%s: %d rows within 1e-9 of a tie" % (case, (~decided).sum())
        assert np.array_equal(lab[decided], want[decided]), case
        assert ulp_diff(resp, g[case + "_resp"]).max() <= 2, case
        # host call (BGMMModel.assign), int64 labels / float32 responsibilities as the reference returns them
        y = m.assign(X)
        assert y.dtype == np.int64 and np.array_equal(y[decided], want[decided])
        r = m.assign(X, values=True)
        assert r.dtype == np.float32 and r.shape == (X.shape[0], m.n_components)
        assert np.array_equal(r, resp)
    # rows whose float32 and float64 quotients x / scale lie on opposite sides of the boundary: the two scale dtypes
    # give different labels there, so a kernel that ignored the stored dtype fails one of the two cases
    n = int(g["split_rows"])
    assert n >= 1 and (g["split_f32_labels"][:n] != g["split_f64_labels"][:n]).all()
    for case in ("split_f32", "split_f64"):
        lab, _ = __import__("poppunk_amd.engine", fromlist=["x"]).bgmm_assign_dev(
            torch.from_numpy(g[case + "_X"]).cuda(), case_model(g, case).model, True, False)
        assert np.array_equal(lab.cpu().numpy()[:n], g[case + "_labels"][:n]), case


def test_host_assign_across_a_chunk_boundary_equals_the_device_path():
    """ppk_bgmm_assign works through its rows in chunks of 8 Mi from one buffer: three rows more than a chunk take the
    loop's second pass, and labels and responsibilities asked for together equal the device-array path's.  The rows
    are the k2 case's, repeated, so both also equal the reference's recorded answers for those rows (an indexing
    error the two paths shared would pass the first comparison alone)."""
    import ctypes as C
    import torch
    from poppunk_amd import _lib, engine
    g = golden()
    m = case_model(g, "k2")
    assert m.n_components == 2
    assert (g["k2_gap"] > 1e-9 * np.maximum(1.0, np.abs(g["k2_top"]))).all()
    n = (8 << 20) + 3
    idx = np.arange(n) % g["k2_X"].shape[0]
    X = np.ascontiguousarray(g["k2_X"][idx])
    lab = np.empty(n, dtype=np.int32)
    resp = np.empty((n, 2), dtype=np.float32)
    rc = _lib.lib().ppk_bgmm_assign(X.ctypes.data_as(C.POINTER(C.c_float)), n, m.model, 0,
                                    lab.ctypes.data_as(C.POINTER(C.c_int32)), resp.ctypes.data_as(C.POINTER(C.c_float)))
    _lib.check(rc, "ppk_bgmm_assign")
    want_lab, want_resp = engine.bgmm_assign_dev(torch.from_numpy(X).cuda(), m.model, True, True)
    assert np.array_equal(lab, want_lab.cpu().numpy())
    assert np.array_equal(resp, want_resp.cpu().numpy())
    assert np.array_equal(lab, g["k2_labels"][idx])
    assert ulp_diff(resp, g["k2_resp"][idx]).max() <= 2


def test_empty_input():
    import torch
    from poppunk_amd import engine
    g = golden()
    lab, resp = engine.bgmm_assign_dev(torch.zeros((0, 2), dtype=torch.float32, device="cuda"),
                                       case_model(g, "k2").model, True, True)
    assert lab.shape == (0,) and resp.shape == (0, 2)


def test_edges_equal_generate_tuples_on_golden_labels():
    import torch
    from poppunk_amd import engine
    g = golden()
    for case in ("k2", "k4", "jitter"):
        m = case_model(g, case)
        X = g[case + "_X"]
        n = 1 + int((1 + np.sqrt(1 + 8 * X.shape[0])) / 2)
        while n * (n - 1) // 2 > X.shape[0]:
            n -= 1
        rows = n * (n - 1) // 2
        Xs = np.ascontiguousarray(X[:rows])
        labels = m.assign(Xs)
        t = torch.from_numpy(Xs).cuda()
        got = engine.bgmm_edges_dev(t, m.model).cpu().numpy()
        assert np.array_equal(got, tuples(labels, m.within_label, True)), case
        got = engine.bgmm_edges_dev(t, m.model, int_offset=7).cpu().numpy()
        assert np.array_equal(got, tuples(labels, m.within_label, True, 0, 7)), case
        n_ref = 37
        rect = (X.shape[0] // n_ref) * n_ref
        Xr = np.ascontiguousarray(X[:rect])
        lab_r = m.assign(Xr)
        tr = torch.from_numpy(Xr).cuda()
        got = engine.bgmm_edges_dev(tr, m.model, n_ref=n_ref, int_offset=11).cpu().numpy()
        assert np.array_equal(got, tuples(lab_r, m.within_label, False, n_ref, 11)), case
        # an 8-byte aligned view (the row-order mask path)
        tv = torch.from_numpy(np.ascontiguousarray(X[: rect + 1])).cuda()[1:]
        got = engine.bgmm_edges_dev(tv, m.model, n_ref=n_ref).cpu().numpy()
        assert np.array_equal(got, tuples(m.assign(X[1:rect + 1]), m.within_label, False, n_ref)), case


def fused_vs_two_step(db, qry, kmers, tbl, m, **kw):
    import torch
    from poppunk_amd import engine
    fused, _ = engine.dist_bgmm_edges(db, qry, kmers, tbl, model=m.model, **kw)
    d, _ = engine.dist(db, qry, kmers, tbl, random_correct=kw.get("random_correct", True))
    lab, _ = engine.bgmm_assign_dev(d, m.model, True, False)
    if qry is None:
        want = engine.generate_tuples_dev(lab, m.within_label, True)
    else:
        want = engine.generate_tuples_dev(lab, m.within_label, False, num_ref=db.n)
    want = want.cpu().numpy()
    q_begin, q_end = kw.get("q_begin", 0), kw.get("q_end", None)
    if q_begin or q_end is not None:
        nq = qry.n if qry is not None else db.n
        q_end = nq if q_end is None else q_end
        if qry is None:
            keep = (want[:, 0] >= q_begin) & (want[:, 0] < q_end)
        else:
            keep = (want[:, 1] - db.n >= q_begin) & (want[:, 1] - db.n < q_end)
        want = want[keep]
    got = fused.cpu().numpy()
    assert np.array_equal(got, want)
    return got.shape[0]


def synth_model(sk_dist, K=2):
    """A model whose within component sits at the close pairs of these sketches (a similar edge fraction to a fit)."""
    from poppunk_amd.models import BGMMModel
    X = sk_dist
    scale = np.amax(X, axis=0)
    scale = np.where(scale > 0, scale, np.float32(1))      # (a column of zeros: nothing to scale)
    Xs = X / scale
    close = np.zeros(Xs.shape[0], dtype=bool)
    close[np.argsort(Xs[:, 0], kind="stable")[: max(3, Xs.shape[0] // 10)]] = True
    mus = [Xs[close].mean(0), Xs[~close].mean(0)]
    covs = [np.cov(Xs[close].T) + 1e-6 * np.eye(2), np.cov(Xs[~close].T) + 1e-6 * np.eye(2)]
    w = [0.1, 0.9]
    for k in range(K - 2):
        mus.append(np.array([0.5 + 0.1 * k, 0.2]))
        covs.append(np.eye(2) * 0.01)
        w.append(0.01)
    w = np.array(w) / np.sum(w)
    return BGMMModel(w, np.array(mus), np.array(covs), scale, 0, 1)


def test_fused_equals_two_step(ppk_option):
    from oracle import oracle
    from poppunk_amd import _lib, engine, synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(700, kmers, cluster_size=25)       # 700: a ragged right edge (not a multiple of 256)
    d, _ = oracle.query(sk[:200], None, kmers, 16, 14, tbl, threads=8)
    for K in (2, 4):
        m = synth_model(d, K)
        db = engine.SketchDB(sk, 16, 14, device=0)
        assert 0 < fused_vs_two_step(db, None, kmers, tbl, m) < db.n * (db.n - 1) // 2
        assert fused_vs_two_step(db, None, kmers, tbl, m, q_begin=128, q_end=448) > 0
        fused_vs_two_step(db, None, kmers, tbl, m, random_correct=False)
        ppk_option("ksplit", 1_000_000)          # the k-split path at this size
        fused_vs_two_step(db, None, kmers, tbl, m)
        ppk_option("ksplit", 0)
        fused_vs_two_step(db, None, kmers, tbl, m)
        ref = engine.SketchDB(sk[:300], 16, 14, device=0)
        qry = engine.SketchDB(sk[300:], 16, 14, device=0)
        assert fused_vs_two_step(ref, qry, kmers, tbl, m) > 0
        for x in (db, ref, qry):
            x.close()
    # the other tile shapes of the fused path: 6 and 9 k-mer lengths (three- and four-dword count registers), and a
    # bbits other than 14 (the generic kernel: 64-bit, 96-bit and 128-bit count packs)
    for kl, bbits, shape in (((13, 15, 17, 19, 21, 23), 14, "v2"), (tuple(range(13, 30, 2)), 14, "v2"),
                             ((13, 17, 21, 25, 29), 16, "generic"), ((13, 15, 17, 19, 21, 23), 16, "generic"),
                             (tuple(range(13, 28, 2)), 16, "generic")):
        kk = np.asarray(kl, dtype=np.int32)
        ksk, _ = synth.make_sketches(300, kk, bbits=bbits, cluster_size=25)
        ktbl = synth.random_match_table(kk)
        kdb = engine.SketchDB(ksk, 16, bbits, device=0)
        kd, _ = engine.dist(kdb, None, kk, ktbl)
        m = synth_model(kd.cpu().numpy()[::7], 2)
        ppk_option("ksplit", 0)
        assert 0 < fused_vs_two_step(kdb, None, kk, ktbl, m)
        engine.dist_bgmm_edges(kdb, None, kk, ktbl, model=m.model)
        assert shape in _lib.lib().ppk_last_kernel_name().decode(), (kl, bbits, _lib.lib().ppk_last_kernel_name())
        kdb.close()
    # a wide k list (k = 6..15, more than 128 count bits at sketchsize64 156)
    wk = np.arange(6, 16, dtype=np.int32)
    wsk, _ = synth.make_sketches(300, wk, sketchsize64=156, bbits=14, cluster_size=15)
    wtbl = synth.random_match_table(wk, genome_length=20_000)
    from poppunk_amd.models import BGMMModel
    m = BGMMModel([0.5, 0.5], [[0.0, 0.0], [0.6, 0.6]], [np.eye(2) * 0.01, np.eye(2) * 0.05],
                  np.float32([0.05, 0.5]), 0, 1)
    db = engine.SketchDB(wsk, 156, 14, device=0)
    for ks in (0, 1200):
        ppk_option("ksplit", ks)
        assert 0 < fused_vs_two_step(db, None, wk, wtbl, m)
    db.close()


def test_host_edges_park_and_pieces(ppk_option):
    from oracle import oracle
    from poppunk_amd import engine, synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(900, kmers, cluster_size=30)
    d, _ = oracle.query(sk[:200], None, kmers, 16, 14, tbl, threads=8)
    m = synth_model(d, 2)
    db = engine.SketchDB(sk, 16, 14, device=0)
    want, _ = m.edges_from_sketches(db, None, kmers, tbl)
    want = want.cpu().numpy()
    got, _ = m.edges_host(db, None, kmers, tbl)
    assert np.array_equal(got, want)
    got, _ = m.edges_host(db, None, kmers, tbl, cap=3)           # parked, then fetched
    assert np.array_equal(got, want)
    got, _ = m.edges_host([db, db], None, kmers, tbl)            # two bands on one device
    assert np.array_equal(got, want)
    ppk_option("chunk_rows", 1)                                  # the smallest pieces
    got, _ = m.edges_host(db, None, kmers, tbl)
    assert np.array_equal(got, want)
    db.close()
