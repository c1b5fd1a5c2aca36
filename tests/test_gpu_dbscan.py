"""GPU tests of the DBSCAN (HDBSCAN) model: core distances and the spanning tree bit for bit against the numpy
restatement of tests/test_dbscan_host.py, fit labels against it and against the committed sklearn labels,
assignment and edge lists label for label, and one full-size fit checked by its own invariants."""
import ctypes as C
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_dbscan_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def dev_fit(P, m):
    from poppunk_amd import engine
    t = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float32)).cuda()
    core2 = engine.dbscan_core_dev(t, m)
    a, b, w = engine.dbscan_mst_dev(t, core2)
    return core2.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy()


def model_from(P, core2, tree, m, c, scale, within=0):
    from poppunk_amd.models import DBSCANModel
    model = DBSCANModel()
    model._set_state(P, core2, tree, m, c)
    model.scale, model.within_label, model.between_label = np.asarray(scale), within, None
    model.n_clusters = tree.n_clusters
    model.fitted = True
    return model


def two_far_blobs(n, seed):
    rng = np.random.default_rng(seed)
    X = np.vstack([rng.normal([0.05, 0.05], 0.01, (n // 2, 2)), rng.normal([0.95, 0.9], 0.01, (n - n // 2, 2))])
    return np.abs(X).astype(np.float32)


# ---- 6. core distances -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,seed,dup", [(300, 10, 0, 0), (300, 10, 1, 120), (40, 39, 2, 0), (65, 1, 3, 10),
                                          (2500, 25, 4, 0), (4500, 1023, 5, 300)])
def test_core_distances_equal_the_restatement_bit_for_bit(n, m, seed, dup):
    from poppunk_amd import engine
    P = H.blobs(n, seed, dup)
    got = engine.dbscan_core_dev(torch.from_numpy(P).cuda(), m).cpu().numpy()
    assert np.array_equal(bits(got), bits(H.ref_core2(P, m)))


def test_core_distance_argument_errors():
    from poppunk_amd import engine
    t = torch.zeros((10, 2), dtype=torch.float32, device="cuda")
    for m in (0, -3, 10):
        with pytest.raises(ValueError):
            engine.dbscan_core_dev(t, m)
    assert np.all(engine.dbscan_core_dev(t, 9).cpu().numpy() == 0.0)


# ---- 7. the spanning tree ----------------------------------------------------------------------------------------------
def mst_cases():
    one = np.tile(np.array([[0.25, 0.5]], dtype=np.float32), (70, 1))
    return [("one point repeated", one, 5), ("many duplicates", H.blobs(400, 1, 250), 8),
            ("two far blobs", two_far_blobs(300, 2), 10), ("plain", H.blobs(500, 3), 10),
            ("across tiles", H.blobs(2600, 4, 100), 26), ("m = n - 1", H.blobs(40, 5), 39)]


@pytest.mark.parametrize("name,P,m", mst_cases(), ids=[c[0] for c in mst_cases()])
def test_spanning_tree_equals_the_restatement_edge_for_edge(name, P, m):
    core2, a, b, w = dev_fit(P, m)
    want_core2 = H.ref_core2(P, m)
    assert np.array_equal(bits(core2), bits(want_core2))
    wa, wb, ww = H.ref_mst(P, want_core2)
    if len(P) <= 500:
        ka, kb, kw = H.ref_mst_kruskal(P, want_core2)
        assert np.array_equal(ka, wa) and np.array_equal(kb, wb) and np.array_equal(bits(kw), bits(ww))
    assert a.dtype == np.int32 and b.dtype == np.int32 and len(a) == len(P) - 1
    assert np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(bits(w), bits(ww))
    if name == "one point repeated":
        assert np.all(w == 0.0) and np.array_equal(a, np.zeros(69)) and np.array_equal(b, np.arange(1, 70))


# ---- 8. fit labels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", H.GOLDEN, ids=[os.path.basename(p) for p in H.GOLDEN])
def test_fit_labels_equal_the_restatement_and_sklearn(path):
    from poppunk_amd import dbscan
    points, m, c, sk, whole = H.load_golden(path)
    core2, a, b, w = dev_fit(points, m)
    tree = dbscan.fit_tree(a, b, w, len(points), c)
    _, mst, want = H.ref_fit(points, m, c)
    assert np.array_equal(tree.labels, want.labels)
    for k in ("pt_cluster", "pt_lambda", "cl_parent", "cl_birth", "cl_label"):
        assert np.array_equal(getattr(tree, k), getattr(want, k)), k
    H.check_against_golden(tree.labels, (a, b, w), points, c, sk, whole, os.path.basename(path))


def test_host_form_of_the_fit():
    from poppunk_amd import _lib
    P = H.blobs(700, 7, 30)
    n, m = len(P), 12
    core2, a, b, w = np.empty(n), np.empty(n - 1, dtype=np.int32), np.empty(n - 1, dtype=np.int32), np.empty(n - 1)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _lib.check(_lib.lib().ppk_dbscan_fit(P.ctypes.data_as(C.POINTER(C.c_float)), n, m, 0, core2.ctypes.data_as(f64p),
                                         a.ctypes.data_as(i32p), b.ctypes.data_as(i32p), w.ctypes.data_as(f64p)))
    d = dev_fit(P, m)
    for got, want in zip((bits(core2), a, b, bits(w)), (bits(d[0]), d[1], d[2], bits(d[3]))):
        assert np.array_equal(got, want)


# ---- 9. assignment -----------------------------------------------------------------------------------------------------
def synth_matrix(n_genomes, cluster_size):
    from poppunk_amd import engine, synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, member = synth.make_sketches(n_genomes, kmers, cluster_size=cluster_size)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    return dist_t, member


def rows_scanned(model):
    from poppunk_amd import _lib
    v = C.c_ulonglong(0)
    _lib.check(_lib.lib().ppk_dbscan_stats(model.handle(0), C.byref(v)), "ppk_dbscan_stats")
    return int(v.value)


def test_assignment_equals_the_restatement_on_a_million_rows(ppk_option):
    dist_t, _ = synth_matrix(2000, 50)
    assert dist_t.shape[0] == 1999000
    X = dist_t.cpu().numpy()
    idx = np.random.default_rng(11).permutation(len(X))[:300]
    scale = np.amax(X[idx], axis=0)
    P = X[idx] / scale
    m, c = 10, 10
    core2, _, tree = H.ref_fit(P, m, c)
    rows = 1 << 20
    t0 = time.perf_counter()
    want = H.ref_assign(H.scale_rows(X[:rows], scale), P, core2, m, tree)
    t1 = time.perf_counter()
    model = model_from(P, core2, tree, m, c, scale)
    print("restatement: %.1f s for %d rows x %d training points; labels used: %s"
          % (t1 - t0, rows, len(P), np.unique(want).tolist()))
    for search in (1, 2):                              # the scan, and the grid in front of it
        ppk_option("dbscan_search", search)
        got = model.assign_dev(dist_t[:rows]).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), search
    print("rows of the grid search that ended as a scan of everything: %d of %d" % (rows_scanned(model), rows))
    # a float64 scale: the float64 quotient meets the training points
    model64 = model_from(P, core2, tree, m, c, scale.astype(np.float64))
    want64 = H.ref_assign(H.scale_rows(X[:50000], scale.astype(np.float64)), P, core2, m, tree)
    assert np.array_equal(model64.assign_dev(dist_t[:50000]).cpu().numpy(), want64)
    # the host form returns int64, as the reference's np.zeros(n, dtype=int)
    y = model.assign(X[:70001])
    assert y.dtype == np.int64 and np.array_equal(y, want[:70001])


@pytest.mark.parametrize("n,m,c,seed", [(200, 10, 10, 0), (120, 5, 6, 1), (15, 10, 3, 2), (2300, 23, 23, 3)])
@pytest.mark.parametrize("search", [0, 1, 2])
def test_assignment_of_planted_rows(n, m, c, seed, search, ppk_option):
    ppk_option("dbscan_search", search)
    P = H.with_index_tie(H.blobs(n, seed, dup=5))
    if n == 200:
        P[30:55] = P[30]                           # w2 = 0 on these
    core2, _, tree = H.ref_fit(P, m, c)
    Q = np.vstack([P, H.planted_rows(P, np.random.default_rng(seed))]).astype(np.float32)
    model = model_from(P, core2, tree, m, c, np.ones(2, dtype=np.float32))
    got = model.assign_dev(torch.from_numpy(Q).cuda()).cpu().numpy()
    want = H.ref_assign(Q.astype(np.float64), P, core2, m, tree)
    assert np.array_equal(got, want)
    # every training point through its own model: the fitted label (the argument is in test_dbscan_host.py), unless
    # it is a repeat of an earlier point
    first = np.array([i == np.flatnonzero((P == P[i]).all(axis=1))[0] for i in range(n)])
    assert np.array_equal(got[:n][first], tree.labels[first])


def test_grid_search_on_a_large_training_set_and_its_fallback_count(ppk_option):
    """5 000 training points (the grid is the default from 1 024 up), rows inside the cloud, on its rim, on training
    points, on cell boundaries and far outside; the scan is the yardstick for all of them, the restatement for a
    sample.  Rows far outside end as a scan of everything and are counted."""
    P = H.blobs(5000, 21, dup=200)
    m, c = 50, 50
    core2, _, tree = H.ref_fit(P, m, c)
    rng = np.random.default_rng(22)
    inside = rng.uniform(0, 1, (60000, 2)).astype(np.float32)
    g = int(np.sqrt(5000 / 4.0))
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    k = rng.integers(0, g + 1, (2000, 2))
    on_cells = (lo + k * ((hi - lo) / g)).astype(np.float32)          # rows on the grid's own lines
    far = np.array([[30.0, 30.0], [-5.0, 0.5], [0.5, 1e6], [1e-30, -1e4]], dtype=np.float32)
    Q = np.vstack([inside, P, on_cells, far, np.float32([[np.inf, 0.5], [np.nan, 0.2]])])
    model = model_from(P, core2, tree, m, c, np.ones(2, dtype=np.float32))
    t = torch.from_numpy(Q).cuda()
    ppk_option("dbscan_search", 1)
    scan = model.assign_dev(t).cpu().numpy()
    before = rows_scanned(model)
    ppk_option("dbscan_search", 0)
    grid = model.assign_dev(t).cpu().numpy()
    assert np.array_equal(grid, scan)
    full = rows_scanned(model) - before
    print("grid: %d of %d rows ended as a scan of everything" % (full, len(Q)))
    assert 6 <= full <= 6 + 60                         # the far and non-finite rows, and at most a few rim rows
    sample = np.concatenate([np.arange(0, len(Q), 37), np.arange(len(Q) - 6, len(Q) - 2)])
    want = H.ref_assign(Q[sample].astype(np.float64), P, core2, m, tree)
    assert np.array_equal(grid[sample], want)
    assert np.array_equal(grid[60000:65000], tree.labels) or len(np.unique(P, axis=0)) < len(P)


def test_host_form_chunk_boundaries():
    P = H.blobs(60, 9)
    m, c = 3, 5
    core2, _, tree = H.ref_fit(P, m, c)
    model = model_from(P, core2, tree, m, c, np.ones(2, dtype=np.float32))
    rows = (4 << 20) + 777                        # one full chunk of the host form and a short one
    Q = np.random.default_rng(3).uniform(-0.1, 1.1, (rows, 2)).astype(np.float32)
    y = model.assign(Q)
    dev = model.assign_dev(torch.from_numpy(Q).cuda()).cpu().numpy()
    assert np.array_equal(y, dev)
    for lo, hi in ((0, 2000), ((4 << 20) - 1000, (4 << 20) + 777)):
        assert np.array_equal(y[lo:hi], H.ref_assign(Q[lo:hi].astype(np.float64), P, core2, m, tree))


# ---- 10. edge lists ----------------------------------------------------------------------------------------------------
def test_edge_lists_equal_assign_then_generate_tuples():
    from poppunk_amd import _lib, engine
    P = H.blobs(300, 4)
    m, c = 10, 10
    core2, _, tree = H.ref_fit(P, m, c)
    assert tree.n_clusters >= 2
    n_samples = 400
    Q = torch.from_numpy(np.random.default_rng(8).uniform(0, 1, (n_samples * (n_samples - 1) // 2, 2))
                         .astype(np.float32)).cuda()
    for within in (0, 1):
        model = model_from(P, core2, tree, m, c, np.array([1.1, 0.9], dtype=np.float32), within=within)
        lab = model.assign_dev(Q)
        want = engine.generate_tuples_dev(lab, within, True, 0, 5).cpu().numpy()
        assert len(want) > 3
        assert np.array_equal(model.edges_dev(Q, int_offset=5).cpu().numpy(), want)
        assert np.array_equal(model.edges_dev(Q, int_offset=5, cap=3).cpu().numpy(), want)   # re-run at the exact size
        # a too-small cap: the total is reported, the first cap pairs are stored
        e = torch.full((3, 2), -7, dtype=torch.int64, device="cuda")
        ne = torch.zeros(1, dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().ppk_dbscan_edges_dev(C.c_void_p(Q.data_ptr()), Q.shape[0], 0, model.handle(0), 5,
                                                   C.c_void_p(e.data_ptr()), 3, C.c_void_p(ne.data_ptr()), None))
        torch.cuda.synchronize()
        assert int(ne.item()) == len(want) and np.array_equal(e.cpu().numpy(), want[:3])
        # ref x query: 50 refs, the rows that divide evenly
        rq = Q[:50 * 300]
        want = engine.generate_tuples_dev(lab[:50 * 300].contiguous(), within, False, 50, 2).cpu().numpy()
        assert np.array_equal(model.edges_dev(rq, n_ref=50, int_offset=2).cpu().numpy(), want)
        assert np.array_equal(np.asarray(model.edges(rq.cpu().numpy(), False, 50, 2), dtype=np.int64).reshape(-1, 2), want)


# ---- 11. end to end ----------------------------------------------------------------------------------------------------
def adjusted_rand(x, y):
    x, y = np.unique(x, return_inverse=True)[1], np.unique(y, return_inverse=True)[1]
    table = np.zeros((x.max() + 1, y.max() + 1))
    np.add.at(table, (x, y), 1)
    comb = lambda v: (v * (v - 1) / 2).sum()     # noqa: E731
    a, b, t, n = comb(table.sum(1)), comb(table.sum(0)), comb(table), len(x)
    expected = a * b / (n * (n - 1) / 2)
    return float((t - expected) / (0.5 * (a + b) - expected))


def test_fit_save_load_edges_clusters(tmp_path):
    from poppunk_amd import distfile, poppunk_refine
    from poppunk_amd.models import DBSCANModel
    # 300 genomes in 5 strains of 60: the generator's within-strain pairs then form a cluster of their own next to
    # the origin (strains of 30 leave too few of them in a 3 000-row subsample, and both sides refuse that fit)
    n_genomes = 300
    dist_t, member = synth_matrix(n_genomes, 60)
    X = dist_t.cpu().numpy()
    args = dict(max_num_clusters=10, min_cluster_prop=0.01, max_samples=3000, seed=7)
    # the yardstick: the restatement on the host copy, the same subsample
    idx = DBSCANModel.subsample_index(len(X), args["max_samples"], args["seed"])
    sub = X[idx].copy()
    scale = np.amax(sub, axis=0)
    sub /= scale
    want = H.ref_model_fit(sub, args["max_num_clusters"], args["min_cluster_prop"])
    model = DBSCANModel()
    y = model.fit_dev(dist_t, **args)
    assert (model.min_samples, model.min_cluster_size) == (want["m"], want["c"])
    assert (model.within_label, model.between_label) == (want["within"], want["between"])
    assert np.array_equal(model.scale, scale) and np.array_equal(model.labels, want["tree"].labels)
    assert np.array_equal(bits(model.core2), bits(want["core2"]))
    want_y = H.ref_assign(H.scale_rows(X, scale), sub, want["core2"], want["m"], want["tree"])
    assert np.array_equal(y.cpu().numpy(), want_y)
    back = DBSCANModel.from_npz(model.save(str(tmp_path / "synth")))
    edges = back.edges_dev(dist_t).cpu().numpy()
    want_edges = np.asarray(poppunk_refine.generateTuples(want_y.astype(np.int64), want["within"], self=True, num_ref=0,
                                                          int_offset=0), dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(edges, want_edges)
    n_comp, comp = distfile.clusters_from_edges(n_genomes, edges)
    n_want, comp_want = distfile.clusters_from_edges(n_genomes, want_edges)
    assert n_comp == n_want and np.array_equal(comp, comp_want)
    print("end to end: %d genomes in %d planted strains -> %d within-strain pairs, %d clusters, adjusted Rand index %.4f"
          % (n_genomes, len(set(member.tolist())), len(edges), n_comp, adjusted_rand(comp, member)))
    # the host entry point gives the same fit from the host copy
    host = DBSCANModel()
    yh = host.fit(X, **args)
    assert np.array_equal(yh, want_y.astype(np.int64)) and np.array_equal(host.labels, model.labels)


def test_dbscan_example_runs_end_to_end(tmp_path):
    """examples/dbscan_fit.py: distances -> fit -> save -> load -> edge list -> clusters."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "dbscan_fit.py"), "300", "60", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "within-strain pairs" in r.stdout and os.path.exists(str(tmp_path / "synthetic_fit.npz"))


# ---- 12. one full-size fit ---------------------------------------------------------------------------------------------
def test_full_size_fit_invariants():
    from poppunk_amd import engine
    n, m = 100000, 1000
    rng = np.random.default_rng(12)
    k = [int(n * 0.03), int(n * 0.07), int(n * 0.88)]
    P = np.vstack([np.abs(rng.normal([0.002, 0.02], [0.001, 0.01], (k[0], 2))),
                   rng.normal([0.012, 0.12], [0.002, 0.03], (k[1], 2)),
                   rng.normal([0.02, 0.3], [0.003, 0.05], (k[2], 2)),
                   rng.uniform(0, [0.03, 0.5], (n - sum(k), 2))]).astype(np.float32)
    P = P[rng.permutation(n)]
    P /= P.max(axis=0)
    t = torch.from_numpy(P).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    core2_t = engine.dbscan_core_dev(t, m)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    a_t, b_t, w_t = engine.dbscan_mst_dev(t, core2_t)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print("full size: core distances %.3f s, spanning tree %.3f s" % (t1 - t0, t2 - t1))
    core2, a, b, w = core2_t.cpu().numpy(), a_t.cpu().numpy().astype(np.int64), b_t.cpu().numpy().astype(np.int64), w_t.cpu().numpy()
    P64 = P.astype(np.float64)
    rows = rng.choice(n, 500, replace=False)
    for r in np.split(rows, 5):                                   # [100, n] float64 blocks
        dx, dy = P64[r, None, 0] - P64[None, :, 0], P64[r, None, 1] - P64[None, :, 1]
        d2 = dx * dx + dy * dy
        d2[np.arange(len(r)), r] = np.inf
        assert np.array_equal(bits(np.partition(d2, m - 1, axis=1)[:, m - 1]), bits(core2[r]))
    del d2, dx, dy

    def key_of(x, y):
        ex, ey = P64[x, 0] - P64[y, 0], P64[x, 1] - P64[y, 1]
        return np.maximum(np.maximum(core2[x], core2[y]), ex * ex + ey * ey)
    assert len(a) == n - 1 and np.all(a < b) and np.all(a >= 0) and np.all(b < n)
    assert np.array_equal(bits(w), bits(key_of(a, b)))
    order = np.lexsort((b, a, w))
    assert np.array_equal(order, np.arange(n - 1))
    # spanning: union-find over the edges leaves one component; the same pass roots the tree for the path queries
    adj_order = np.argsort(np.concatenate([a, b]), kind="stable")
    ends = np.concatenate([b, a])[adj_order]
    eidx = np.concatenate([np.arange(n - 1), np.arange(n - 1)])[adj_order]
    start = np.searchsorted(np.concatenate([a, b])[adj_order], np.arange(n + 1))
    parent, pedge, depth = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    depth[0], frontier, seen = 0, np.array([0]), 1
    while len(frontier):
        nxt = []
        for v in frontier.tolist():
            for u, e in zip(ends[start[v]:start[v + 1]].tolist(), eidx[start[v]:start[v + 1]].tolist()):
                if depth[u] < 0:
                    depth[u], parent[u], pedge[u] = depth[v] + 1, v, e
                    nxt.append(u)
        seen += len(nxt)
        frontier = np.array(nxt, dtype=np.int64)
    assert seen == n                                              # n - 1 edges reaching every point: a spanning tree
    # the cycle property on 200 pairs that are not tree edges: under the total order (position in the sorted list
    # for tree edges) the pair lies above every edge on the tree path between its ends
    tree_pairs = set(zip(a.tolist(), b.tolist()))
    checked = 0
    while checked < 200:
        x, y = sorted(rng.choice(n, 2, replace=False).tolist())
        if (x, y) in tree_pairs:
            continue
        kw = float(key_of(np.array([x]), np.array([y]))[0])
        top, u, v = -1, x, y
        while u != v:
            if depth[u] < depth[v]:
                u, v = v, u
            top, u = max(top, int(pedge[u])), int(parent[u])
        assert (kw, x, y) > (float(w[top]), int(a[top]), int(b[top]))
        checked += 1
