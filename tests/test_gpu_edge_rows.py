"""Fused edge lists that carry their distances, on a real MI355X (ppk_dist_edges_rows_dev).

The contract is bit equality with what exists: the edges are dist_edges' (or dist_bgmm_edges'), and row e is the row
the dense kernel writes for edge e -- torch.equal on an integer view against engine.dist(...)[rows of the edges], same
databases, k list, table and options.  Every case runs on the route the job takes by default (at these sizes the k-split
kernels, i.e. the two-step) AND with option "ksplit" 0, which sends it through whole tiles: the rows modes of the tile
kernel.  ppk_last_kernel_name() says which ran."""
import ctypes as C

import numpy as np
import pytest

from poppunk_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
NOTHING, EVERYTHING = (1e-6, 1e-6), (10.0, 10.0)


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dense_rows(edges_t, n_ref, n_qry=0):
    """Rows of the whole job's dense result that the edges (i < j; ref x query: (r, n_ref + q)) stand for."""
    a, b = edges_t[:, 0], edges_t[:, 1]
    if n_qry:
        return (b - n_ref) * n_ref + a
    return a * n_ref - (a * (a + 1)) // 2 + (b - a - 1)


def _kernel():
    return _lib.lib().ppk_last_kernel_name().decode()


def _check(ref, qry, tbl, dense, fused=None, kmers=KMERS, **kw):
    """dist_edges_rows against dist_edges + the dense rows, twice.  fused: True / False asserts which path ran."""
    import torch
    e0, f0 = engine.dist_edges(ref, qry, kmers, tbl, **kw)
    e1, r1, f1 = engine.dist_edges_rows(ref, qry, kmers, tbl, **kw)
    name = _kernel()
    assert torch.equal(e0, e1) and int(f0.item()) == int(f1.item())
    assert r1.shape == (e1.shape[0], 2) and r1.dtype == torch.float32
    assert _same(r1, dense[_dense_rows(e1, ref.n, qry.n if qry is not None else 0)])
    e2, r2, f2 = engine.dist_edges_rows(ref, qry, kmers, tbl, **kw)
    assert torch.equal(e1, e2) and _same(r1, r2) and int(f2.item()) == int(f1.item())
    if fused is True:
        assert ",rows>" in name and "pairs list" not in name, name
    if fused is False and e1.shape[0]:
        assert "pairs list" in name and ",rows>" not in name, name
    return e1, r1


@pytest.fixture(scope="module")
def set300():
    """n = 300 clustered genomes, s = 1 024, the default k list: sketches, table, database, dense result."""
    sk, member = synth.make_sketches(300, KMERS, cluster_size=30)
    tbl = synth.random_match_table(KMERS)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dense, failed = engine.dist(db, None, KMERS, tbl)
    return {"sk": sk, "member": member, "tbl": tbl, "db": db, "dense": dense, "failed": int(failed.item())}


@pytest.mark.parametrize("route", ["default", "tiles"])
@pytest.mark.parametrize("n", [65, 257, 300])
def test_self_shapes(n, route, set300, ppk_option):
    """Ragged against the 64-lane word (65), the 256 x 32 tile (257) and both (300); three boundaries each."""
    if route == "tiles":
        ppk_option("ksplit", 0)
    tbl = set300["tbl"]
    db = engine.SketchDB(set300["sk"][:n], 16, 14, device=0)
    dense, _ = engine.dist(db, None, KMERS, tbl)
    total = n * (n - 1) // 2
    x2, y2 = synth.boundary_for_quantile(dense.cpu().numpy(), 0.02)
    fused = True if route == "tiles" else None
    e, _ = _check(db, None, tbl, dense, fused, x_max=NOTHING[0], y_max=NOTHING[1])
    assert e.shape[0] == 0
    e, _ = _check(db, None, tbl, dense, fused, x_max=x2, y_max=y2)
    assert 0 < e.shape[0] < total // 8
    e, _ = _check(db, None, tbl, dense, fused, x_max=EVERYTHING[0], y_max=EVERYTHING[1])
    assert e.shape[0] == total
    db.close()


@pytest.mark.parametrize("route", ["default", "tiles"])
def test_ref_query_and_bands(route, set300, ppk_option):
    if route == "tiles":
        ppk_option("ksplit", 0)
    sk, tbl = set300["sk"], set300["tbl"]
    n_ref, n_qry = 70, 130
    rdb, qdb = engine.SketchDB(sk[:n_ref], 16, 14), engine.SketchDB(sk[n_ref:n_ref + n_qry], 16, 14)
    dense, _ = engine.dist(rdb, qdb, KMERS, tbl)
    x2, y2 = synth.boundary_for_quantile(dense.cpu().numpy(), 0.1)
    fused = True if route == "tiles" else None
    whole, _ = _check(rdb, qdb, tbl, dense, fused, x_max=x2, y_max=y2)
    assert 0 < whole.shape[0] < n_ref * n_qry
    bounds = engine.band_split(n_ref, n_qry, 2)
    assert 0 < bounds[1] < n_qry
    got = 0
    for lo, hi in ((bounds[0], bounds[1]), (bounds[1], bounds[2]), (64, 101)):
        e, _ = _check(rdb, qdb, tbl, dense, fused, x_max=x2, y_max=y2, q_begin=lo, q_end=hi)
        q = e[:, 1] - n_ref
        assert bool(((q >= lo) & (q < hi)).all())
        got += e.shape[0] if (lo, hi) != (64, 101) else 0
    assert got == whole.shape[0]
    _check(rdb, qdb, tbl, dense, fused, x_max=EVERYTHING[0], y_max=EVERYTHING[1], q_begin=64, q_end=101)
    # a band of a self job: rows [64, 200) of the triangle
    e, _ = _check(set300["db"], None, tbl, set300["dense"], fused, x_max=x2, y_max=y2, q_begin=64, q_end=200)
    assert e.shape[0] > 0 and bool(((e[:, 0] >= 64) & (e[:, 0] < 200)).all())


@pytest.mark.parametrize("route", ["default", "tiles"])
def test_inclusive_against_exclusive_and_scale(route, set300, ppk_option):
    if route == "tiles":
        ppk_option("ksplit", 0)
    db, tbl, dense = set300["db"], set300["tbl"], set300["dense"]
    fused = True if route == "tiles" else None
    core = np.sort(dense[:, 0].cpu().numpy())
    x_on = float(core[core.size // 10])          # a core value that occurs: rows lie ON the slope-0 line
    e_in, r_in = _check(db, None, tbl, dense, fused, slope=0, x_max=x_on, y_max=0.0, inclusive=True)
    e_ex, r_ex = _check(db, None, tbl, dense, fused, slope=0, x_max=x_on, y_max=0.0, inclusive=False)
    on_line = int((dense[:, 0] == x_on).sum().item())
    assert on_line >= 1 and e_in.shape[0] - e_ex.shape[0] == on_line
    assert float(r_in[:, 0].max().item()) == x_on and float(r_ex[:, 0].max().item()) < x_on
    x2, y2 = synth.boundary_for_quantile(dense.cpu().numpy(), 0.05)
    for slope in (1, 2):
        for inclusive in (True, False):
            e, _ = _check(db, None, tbl, dense, fused, slope=slope, x_max=x2, y_max=y2, inclusive=inclusive)
            assert e.shape[0] > 0
    # the scales enter the test only: the rows come out unscaled
    sx, sy = 0.37, 1.9
    e_s, r_s = _check(db, None, tbl, dense, fused, x_max=x2 / sx, y_max=y2 / sy, scale=(sx, sy))
    assert e_s.shape[0] > 0 and _same(r_s, dense[_dense_rows(e_s, 300)])


def _raw(db, tbl, x_max, y_max, cap):
    """ppk_dist_edges_rows_dev as it is, with a cap of the caller's: (edges, rows, n_edges)."""
    import torch
    edges = torch.full((max(cap, 1), 2), -1, dtype=torch.int64, device="cuda:0")
    rows = torch.empty((max(cap, 1), 2), dtype=torch.float32, device="cuda:0")
    n_edges = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    n_failed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    tbl = np.ascontiguousarray(tbl, dtype=np.float32)
    engine._dev_call("ppk_dist_edges_rows_dev", 0, db._h, None, KMERS, tbl, 1, engine.FLAG_RANDOM_CORRECT, 0, db.n, 2,
                     float(x_max), float(y_max), 1.0, 1.0, 1, edges, rows, cap, n_edges, n_failed)
    torch.cuda.synchronize()
    return edges, rows, int(n_edges.item())


@pytest.mark.parametrize("route", ["default", "tiles"])
def test_short_cap(route, set300, ppk_option):
    import torch
    if route == "tiles":
        ppk_option("ksplit", 0)
    db, tbl, dense = set300["db"], set300["tbl"], set300["dense"]
    x2, y2 = synth.boundary_for_quantile(dense.cpu().numpy(), 0.05)
    want, _ = engine.dist_edges(db, None, KMERS, tbl, x_max=x2, y_max=y2)
    total = want.shape[0]
    assert total > 200
    for cap in (0, 1, 100, total - 1):
        edges, _, n = _raw(db, tbl, x2, y2, cap)
        assert n == total
        assert torch.equal(edges[:cap], want[:cap])
        assert cap == 0 or bool((edges[cap:] == -1).all())
    edges, rows, n = _raw(db, tbl, x2, y2, total)
    assert n == total and torch.equal(edges, want) and _same(rows, dense[_dense_rows(want, 300)])
    # the wrapper's second run is exact
    e, r, _ = engine.dist_edges_rows(db, None, KMERS, tbl, x_max=x2, y_max=y2, cap=100)
    assert torch.equal(e, want) and _same(r, dense[_dense_rows(want, 300)])
    # argument errors: dist_edges_dev's, and a missing row buffer
    k = np.ascontiguousarray(KMERS)
    t = np.ascontiguousarray(tbl, dtype=np.float32)
    ne = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def call(slope, d_rows, d_n):
        return _lib.lib().ppk_dist_edges_rows_dev(
            db._h, None, k.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_float)), 1,
            engine.FLAG_RANDOM_CORRECT, 0, db.n, slope, x2, y2, 1.0, 1.0, 1, C.c_void_p(edges.data_ptr()), d_rows,
            total, d_n, None, None)
    assert call(2, None, C.c_void_p(ne.data_ptr())) == _lib.ERR_ARG
    assert call(3, C.c_void_p(rows.data_ptr()), C.c_void_p(ne.data_ptr())) == _lib.ERR_ARG
    assert call(2, C.c_void_p(rows.data_ptr()), None) == _lib.ERR_ARG


@pytest.mark.parametrize("route", ["default", "tiles"])
def test_failed_pairs_and_two_cluster_table(route, set300, ppk_option):
    if route == "tiles":
        ppk_option("ksplit", 0)
    fused = True if route == "tiles" else None
    # unrelated samples: different-cluster pairs match by chance only, fewer than 2 usable k, rows (0, 0).  600 of them:
    # whole 256 x 32 tiles away from the diagonal, whose wavefronts start on the epilogue's table path and leave it at
    # the first pair without a fit
    sk, _ = synth.make_sketches(600, KMERS, cluster_size=20, related=False)
    tbl = synth.random_match_table(KMERS)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dense, failed = engine.dist(db, None, KMERS, tbl)
    n_failed = int(failed.item())
    zero = (dense == 0).all(dim=1)
    assert 0 < n_failed < dense.shape[0] and int(zero.sum().item()) == n_failed
    e, r = _check(db, None, tbl, dense, fused, x_max=EVERYTHING[0], y_max=EVERYTHING[1])
    assert e.shape[0] == dense.shape[0] and int((r == 0).all(dim=1).sum().item()) == n_failed
    _, _, f = engine.dist_edges_rows(db, None, KMERS, tbl, x_max=EVERYTHING[0], y_max=EVERYTHING[1])
    assert int(f.item()) == n_failed
    db.close()
    # a random table with two clusters, not symmetric: the orientation of a pair matters
    tbl2 = synth.random_match_table(KMERS, n_clu=2)
    tbl2 = (tbl2 * np.random.Generator(np.random.PCG64(11)).uniform(0.5, 3.0, size=tbl2.shape)).astype(np.float32)
    assert not np.array_equal(tbl2, tbl2.transpose(0, 2, 1))
    clu = (set300["member"] % 2).astype(np.uint16)
    db2 = engine.SketchDB(set300["sk"], 16, 14, clusters=clu)
    dense2, _ = engine.dist(db2, None, KMERS, tbl2)
    assert not _same(dense2, set300["dense"])
    x2, y2 = synth.boundary_for_quantile(dense2.cpu().numpy(), 0.05)
    e, _ = _check(db2, None, tbl2, dense2, fused, x_max=x2, y_max=y2)
    assert e.shape[0] > 0
    _check(db2, None, tbl2, dense2, fused, x_max=EVERYTHING[0], y_max=EVERYTHING[1])
    db2.close()


ROUTES = {
    # name: (options, whether the rows come out of the tile kernel's epilogue (None: whatever the route choice says))
    "default": ({}, None),
    "tiles": ({"ksplit": 0}, True),
    "tiles_raw_planes": ({"ksplit": 0, "rank_planes": 0}, True),
    "tiles_two_step": ({"ksplit": 0, "edge_rows_fused": 0}, False),
    "ksplit": ({"ksplit": 1_000_000}, False),
    "wide": ({"ksplit": 0, "wide_kpg": 2}, False),
    "wide_ksplit": ({"ksplit": 1_000_000, "wide_kpg": 2}, False),
    "fit_skip_on": ({"ksplit": 0, "ext_fit_skip": 1}, True),
    "fit_skip_off": ({"ksplit": 0, "ext_fit_skip": 0}, True),
}


@pytest.fixture(scope="module")
def sk600():
    """600 clustered genomes: whole 256 x 32 tiles away from the diagonal, which fit from the table in LDS."""
    return synth.make_sketches(600, KMERS, cluster_size=30)[0]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes(route, set300, sk600, ppk_option):
    options, fused = ROUTES[route]
    for name, value in options.items():
        ppk_option(name, value)
    tbl = set300["tbl"]
    # (a database of its own: the coded copies a self job reads are made under the options in force)
    db = engine.SketchDB(sk600, 16, 14, device=0)
    dense, _ = engine.dist(db, None, KMERS, tbl)
    x2, y2 = synth.boundary_for_quantile(dense.cpu().numpy(), 0.02)
    e, _ = _check(db, None, tbl, dense, fused, x_max=x2, y_max=y2)
    assert e.shape[0] > 0
    _check(db, None, tbl, dense, fused, x_max=EVERYTHING[0], y_max=EVERYTHING[1])
    db.close()


def test_three_and_four_dword_count_registers(ppk_option):
    """6 and 9 k-mer lengths: the W = 3 and W = 4 instantiations of the rows modes (no LDS table: the general epilogue)."""
    ppk_option("ksplit", 0)
    for kl in ((13, 15, 17, 19, 21, 23), tuple(range(13, 30, 2))):
        kk = np.asarray(kl, dtype=np.int32)
        sk, _ = synth.make_sketches(300, kk, cluster_size=30)
        tbl = synth.random_match_table(kk)
        db = engine.SketchDB(sk, 16, 14, device=0)
        dense, _ = engine.dist(db, None, kk, tbl)
        x2, y2 = synth.boundary_for_quantile(dense.cpu().numpy(), 0.05)
        e, _ = _check(db, None, tbl, dense, True, kmers=kk, x_max=x2, y_max=y2)
        assert e.shape[0] > 0
        _check(db, None, tbl, dense, True, kmers=kk, x_max=EVERYTHING[0], y_max=EVERYTHING[1])
        db.close()


def _bgmm_model(dense_np, K):
    """A model whose within component sits at the close pairs (tests/test_gpu_bgmm.py's synth_model)."""
    from poppunk_amd.models import BGMMModel
    scale = np.amax(dense_np, axis=0)
    Xs = dense_np / scale
    close = np.zeros(Xs.shape[0], dtype=bool)
    close[np.argsort(Xs[:, 0], kind="stable")[: max(3, Xs.shape[0] // 10)]] = True
    mus = [Xs[close].mean(0), Xs[~close].mean(0)]
    covs = [np.cov(Xs[close].T) + 1e-6 * np.eye(2), np.cov(Xs[~close].T) + 1e-6 * np.eye(2)]
    w = [0.1, 0.9]
    for k in range(K - 2):
        mus.append(np.array([0.5 + 0.1 * k, 0.2]))
        covs.append(np.eye(2) * 0.01)
        w.append(0.01)
    return BGMMModel(np.array(w) / np.sum(w), np.array(mus), np.array(covs), scale, 0, 1)


@pytest.mark.parametrize("route", ["default", "tiles"])
@pytest.mark.parametrize("K", [2, 3])
def test_bgmm(K, route, set300, ppk_option):
    import torch
    if route == "tiles":
        ppk_option("ksplit", 0)
    db, tbl, dense, sk = set300["db"], set300["tbl"], set300["dense"], set300["sk"]
    m = _bgmm_model(dense.cpu().numpy(), K)
    jobs = [(db, None, dense, {}), (db, None, dense, {"q_begin": 64, "q_end": 200})]
    rdb, qdb = engine.SketchDB(sk[:170], 16, 14), engine.SketchDB(sk[170:], 16, 14)
    jobs.append((rdb, qdb, engine.dist(rdb, qdb, KMERS, tbl)[0], {}))
    for ref, qry, d, kw in jobs:
        e0, f0 = engine.dist_bgmm_edges(ref, qry, KMERS, tbl, model=m.model, **kw)
        e1, r1, f1 = engine.dist_bgmm_edges_rows(ref, qry, KMERS, tbl, model=m.model, **kw)
        name = _kernel()
        assert 0 < e0.shape[0] < d.shape[0]
        assert torch.equal(e0, e1) and int(f0.item()) == int(f1.item())
        assert _same(r1, d[_dense_rows(e1, ref.n, qry.n if qry is not None else 0)])
        e2, r2, _ = engine.dist_bgmm_edges_rows(ref, qry, KMERS, tbl, model=m.model, **kw)
        assert torch.equal(e1, e2) and _same(r1, r2)
        if route == "tiles":
            assert ",rows>" in name and "pairs list" not in name, name


def test_weights_of_rows(set300, ppk_option):
    ppk_option("ksplit", 0)
    db, tbl, dense = set300["db"], set300["tbl"], set300["dense"]
    x_max, y_max = synth.boundary_for_quantile(dense.cpu().numpy(), 0.08)
    edges, rows, _ = engine.dist_edges_rows(db, None, KMERS, tbl, x_max=x_max, y_max=y_max)
    assert 1000 < edges.shape[0] < 10000
    for kind in ("core", "accessory", "euclidean"):
        want = engine.edge_weights_from_sketches(db, None, KMERS, tbl, edges, kind)
        assert _same(engine.edge_weights_of_rows(rows, kind), want), kind
        assert _same(want, engine.edge_weights_dev(dense, edges, kind)), kind
    with pytest.raises(ValueError):
        engine.edge_weights_of_rows(rows, "jaccard")
