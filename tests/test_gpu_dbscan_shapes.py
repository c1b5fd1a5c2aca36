"""GPU tests of the shapes of ppk_dbscan.hip that tests/test_gpu_dbscan.py never reaches: tiles of
2, 3, 2 048 and 2 049 points, ranks up to n - 1, d2 over 200 binades, lattices that tie at the rank; Boruvka on chains
that hook into one deep tree, on lattices and constant core distances that tie across tiles; the assignment on a grid
of more than 64 rows at m = 1023, up a condensed tree hundreds of clusters deep, on degenerate bounding boxes, at the
default switch between scan and grid, and at row counts that fill no wave or workgroup.

The inputs come from tests/dbscan_shapes.py, and tests/test_dbscan_host.py proves on the CPU that each reaches the
branch it was built for.  The references are the restatements of tests/test_dbscan_host.py.  Every comparison is
exact: integers element for element, doubles by bit pattern."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dbscan_shapes as S  # noqa: E402
import test_dbscan_host as H  # noqa: E402
from test_gpu_dbscan import bits, dev_fit, model_from, rows_scanned  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

ONES = np.ones(2, dtype=np.float32)


def dev_mst(P, core2):
    from poppunk_amd import engine
    t = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float32)).cuda()
    a, b, w = engine.dbscan_mst_dev(t, torch.from_numpy(np.ascontiguousarray(core2, dtype=np.float64)).cuda())
    return a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy()


def assign(model, Q):
    return model.assign_dev(torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()).cpu().numpy()


def synthetic(P, n_cl, m, seed, scale=ONES):
    M = S.synthetic_model(len(P), n_cl, np.random.default_rng(seed), points=P)
    return M, model_from(M.points, M.core2, M, m, m, scale)


# ---- core distances ----------------------------------------------------------------------------------------------------
def core_points(kind, n):
    if kind == "blobs":
        return H.blobs(n, 100 + n)
    return S.wide_range(n, 0) if kind == "wide" else S.lattice(33)


@pytest.mark.parametrize("kind,n,m", [("blobs", 2, 1), ("blobs", 3, 1), ("blobs", 3, 2), ("blobs", 64, 63), ("blobs", 128, 1),
                                      ("blobs", 2048, 1), ("blobs", 2048, 2047), ("blobs", 2049, 1),
                                      ("blobs", 2049, 2048), ("blobs", 4097, 10), ("wide", 2049, 7),
                                      ("lattice", 1089, 4), ("lattice", 1089, 8)])
def test_core_distances_at_tile_edges_ranks_and_exponents(kind, n, m):
    from poppunk_amd import engine
    P = core_points(kind, n)
    assert len(P) == n
    got = engine.dbscan_core_dev(torch.from_numpy(P).cuda(), m).cpu().numpy()
    want = H.ref_core2(P, m)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:8]


# ---- the spanning tree -------------------------------------------------------------------------------------------------
def check_tree(P, core2, got):
    a, b, w = got
    wa, wb, ww = H.ref_mst(P, core2)
    if len(P) <= 514:
        ka, kb, kw = H.ref_mst_kruskal(P, core2)
        assert np.array_equal(ka, wa) and np.array_equal(kb, wb) and np.array_equal(bits(kw), bits(ww))
    assert a.dtype == np.int32 and b.dtype == np.int32 and len(a) == len(P) - 1
    assert np.array_equal(a, wa), np.flatnonzero(a != wa)[:8]
    assert np.array_equal(b, wb), np.flatnonzero(b != wb)[:8]
    assert np.array_equal(bits(w), bits(ww))


def fit_and_check_tree(P, m):
    core2, a, b, w = dev_fit(P, m)
    want_core2 = H.ref_core2(P, m)
    assert np.array_equal(bits(core2), bits(want_core2))
    check_tree(P, want_core2, (a, b, w))
    return a, b, w


@pytest.mark.parametrize("n", [2, 3, 1024, 1025, 2049])
def test_spanning_tree_at_tile_edges(n):
    fit_and_check_tree(H.blobs(n, 200 + n), min(5, n - 1))


@pytest.mark.parametrize("n", [16, 34, 514, 4096])
def test_spanning_tree_of_two_chains_needs_every_jump_pass(n):
    """Round one hooks each chain into one tree about n / 2 deep (1, 3, 3 and 3 pointer-jumping passes of 16 hops
    for these n); the second round joins the two only if every point then carries its root."""
    P = S.two_chains(n)
    assert np.array_equal(S.least_partner(P, H.ref_core2(P, 1)), S.chain_successors(n))
    a, b, _ = fit_and_check_tree(P, 1)
    h = n // 2
    inside = np.concatenate([np.arange(h - 1), np.arange(h, n - 1)])
    cross = (a < h) != (b < h)
    assert cross.sum() == 1                                                      # the two paths and one joining edge
    assert np.array_equal(np.sort(a[~cross]), inside) and np.array_equal(b[~cross], a[~cross] + 1)


@pytest.mark.parametrize("s", [22, 33])
def test_spanning_tree_of_a_lattice(s):
    fit_and_check_tree(S.lattice(s), 4)


def test_spanning_tree_over_200_binades():
    fit_and_check_tree(S.wide_range(2049, 0), 7)


def test_spanning_tree_from_given_core_distances():
    P = H.blobs(2600, 4, 100)
    n = len(P)
    # every edge ties at 4.0 (every d2 is below it): the order alone decides, and the tree is the star of point 0
    const = np.full(n, 4.0)
    a, b, w = dev_mst(P, const)
    check_tree(P, const, (a, b, w))
    assert np.array_equal(a, np.zeros(n - 1)) and np.array_equal(b, np.arange(1, n)) and np.all(w == 4.0)
    # no core distance at all: the plain Euclidean tree
    check_tree(P, np.zeros(n), dev_mst(P, np.zeros(n)))
    # one point repeated over more than one tile of the nearest kernel
    one = np.tile(np.array([[0.25, 0.5]], dtype=np.float32), (1100, 1))
    a, b, w = dev_mst(one, np.zeros(1100))
    assert np.array_equal(a, np.zeros(1099)) and np.array_equal(b, np.arange(1, 1100))
    assert np.array_equal(bits(w), np.zeros(1099, dtype=np.uint64))


# ---- assignment --------------------------------------------------------------------------------------------------------
SCANNED_FAR_ROWS = {"low": [0, 1, 3], "top": [0, 2, 3]}


@pytest.mark.parametrize("blob", ["low", "top"])
def test_grid_of_more_than_64_rows_at_the_largest_min_samples(blob, ppk_option):
    """20 000 training points (g = 70) and m = 1023: a row in the thin background needs a square of more than 64
    grid rows, where the lanes' strided count of the square's grid rows runs a second time.  Set A certifies in that
    square with 10 % to spare and is never scanned; set B (the whole grid at once, far outside, not finite) always is.
    With the blob against the upper edge ("top") it lies in the grid rows past the 64th of every square of set A: a
    count that left them out would grow those squares into the whole grid, and the rows would be counted as scanned.
    One far row of each input is not in set B: its first square spans the grid in one direction, only one side has
    cells beyond it, and it certifies there."""
    P, rows = S.tall_grid_points(blob)
    m = S.TALL_M
    G = S.grid_of(P)
    assert G.g == 70
    A, tall, whole = S.tall_grid_row_sets(G, rows, m)
    far = S.scanned_far_rows(G, m)
    assert far == SCANNED_FAR_ROWS[blob]
    decided = sum(S.rows_past_the_64th_decide(G, rows[i].astype(np.float64), m) for i in A)
    assert decided == (len(A) if blob == "top" else 0)
    Q = np.vstack([rows, S.FAR_ROWS, S.NON_FINITE_ROWS])
    n_finite = len(rows) + len(S.FAR_ROWS)
    B = np.concatenate([whole, len(rows) + np.array(far), n_finite + np.arange(len(S.NON_FINITE_ROWS))])
    print("%s, first 1500 rows: %d with a first square of more than 64 grid rows, set A %d, whole grid at once %d; set B %d"
          % (blob, len(tall), len(A), len(whole), len(B)))
    assert len(A) > 0 and len(whole) > 0
    M, model = synthetic(P, 400, m, 32)
    ppk_option("dbscan_search", 2)
    before = rows_scanned(model)
    got_a = assign(model, Q[A])
    delta_a = rows_scanned(model) - before
    got_b = assign(model, Q[B])
    delta_b = rows_scanned(model) - before - delta_a
    print("rows scanned: set A %d of %d, set B %d of %d" % (delta_a, len(A), delta_b, len(B)))
    assert delta_a == 0
    assert delta_b == len(B)
    grid = assign(model, Q)
    ppk_option("dbscan_search", 1)
    scan = assign(model, Q)
    assert np.array_equal(grid, scan), np.flatnonzero(grid != scan)[:8]
    assert np.array_equal(got_a, grid[A]) and np.array_equal(got_b, grid[B])
    # (rows that are not finite have no label by the definition: the two searches agree on them, above)
    rest = np.setdiff1d(np.arange(n_finite), A[:300])
    sample = np.concatenate([A[:300], rest[::len(rest) // 300], B[B < n_finite]])
    want = H.ref_assign(Q[sample].astype(np.float64), P, M.core2, m, M, block=128)
    assert np.array_equal(grid[sample], want), sample[np.flatnonzero(grid[sample] != want)[:8]]
    assert len(np.unique(want)) >= 5
    # a float64 scale through the grid: the float64 quotient meets the training points
    scale = np.array([1.1, 0.9])
    A64, _, _ = S.tall_grid_row_sets(G, rows, m, scale=scale)
    assert len(A64) > 0
    model64 = model_from(M.points, M.core2, M, m, m, scale)
    scan64 = assign(model64, Q)
    ppk_option("dbscan_search", 2)
    before = rows_scanned(model64)
    got_a = assign(model64, Q[A64])
    assert rows_scanned(model64) == before
    grid64 = assign(model64, Q)
    assert np.array_equal(grid64, scan64) and np.array_equal(got_a, grid64[A64])
    sample = np.concatenate([A64[:100], np.arange(0, len(rows), 67), np.arange(len(rows), n_finite)])
    want = H.ref_assign(H.scale_rows(Q[sample], scale), P, M.core2, m, M, block=128)
    assert np.array_equal(grid64[sample], want)


@pytest.mark.parametrize("n,n_cl", [(300, 200), (2300, 500)])
@pytest.mark.parametrize("search", [0, 1, 2])
def test_assignment_walks_a_deep_condensed_tree(n, n_cl, search, ppk_option):
    ppk_option("dbscan_search", search)
    m = 10
    M = S.synthetic_model(n, n_cl, np.random.default_rng(n))
    model = model_from(M.points, M.core2, M, m, m, ONES)
    Q = np.vstack([M.points, H.planted_rows(M.points, np.random.default_rng(1)),
                   np.random.default_rng(2).uniform(-3, 4, (200, 2)).astype(np.float32)])
    depth = max(S.walk_depth(q, M, m) for q in Q[n:].astype(np.float64))
    assert depth >= n_cl // 4                       # some row climbs a good part of the chain of n_cl // 2 clusters
    want = H.ref_assign(Q.astype(np.float64), M.points, M.core2, m, M)
    got = assign(model, Q)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert len(np.unique(want)) == 6


@pytest.mark.parametrize("search", [1, 2])
def test_assignment_at_the_largest_min_samples(search, ppk_option):
    """m = 1023 on 2 300 points: rank_k = 2045, and the grid's target is every point.  The fitted model is what
    PopPUNK's rule would make of these points (all noise at this m); the drawn model on the same points has labels
    that tell the neighbours apart."""
    ppk_option("dbscan_search", search)
    P = H.with_index_tie(H.blobs(2300, 3, dup=5))
    m, c = 1023, 23
    core2, _, tree = H.ref_fit(P, m, c)
    Q = np.vstack([P, H.planted_rows(P, np.random.default_rng(3))]).astype(np.float32)
    got = assign(model_from(P, core2, tree, m, c, ONES), Q)
    assert np.array_equal(got, H.ref_assign(Q.astype(np.float64), P, core2, m, tree))
    M, model = synthetic(P, 300, m, 7)
    want = H.ref_assign(Q.astype(np.float64), P, M.core2, m, M)
    got = assign(model, Q)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert len(np.unique(want)) >= 5


@pytest.mark.parametrize("n", [2048, 2049])
@pytest.mark.parametrize("search", [1, 2])
def test_assignment_at_the_scan_tile_edge(n, search, ppk_option):
    ppk_option("dbscan_search", search)
    P = H.blobs(n, 40 + n)
    m, c = 10, 20
    core2, _, tree = H.ref_fit(P, m, c)
    assert tree.n_clusters >= 2
    Q = np.vstack([P, H.planted_rows(P, np.random.default_rng(n))]).astype(np.float32)
    got = assign(model_from(P, core2, tree, m, c, ONES), Q)
    want = H.ref_assign(Q.astype(np.float64), P, core2, m, tree)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def degenerate_points(kind):
    t = np.random.default_rng(5).uniform(0, 1, 400).astype(np.float32)
    if kind == "vertical line":
        return np.stack([np.full(400, 0.5, dtype=np.float32), t], axis=1)
    if kind == "horizontal line":
        return np.stack([t, np.full(400, 0.25, dtype=np.float32)], axis=1)
    return np.tile(np.array([[0.25, 0.5]], dtype=np.float32), (400, 1))


@pytest.mark.parametrize("kind", ["vertical line", "horizontal line", "one point"])
def test_assignment_on_a_degenerate_bounding_box(kind, ppk_option):
    """A box with no width has cells of width 1.0 in that direction (both, for one point repeated): every training
    point is in the first of them.  Rows on the line, beside it, far from it and on training points, through the grid,
    the scan and the restatement; a fitted model, and a drawn one whose labels tell the neighbours apart."""
    P = degenerate_points(kind)
    G = S.grid_of(P)
    assert G.g == 10 and (G.wx == 1.0 or G.wy == 1.0) and ((G.wx == 1.0 and G.wy == 1.0) == (kind == "one point"))
    rng = np.random.default_rng(6)
    t = rng.uniform(-0.2, 1.2, 60).astype(np.float32)
    off = np.float32([0.0, 1e-6, -1e-6, 0.01, -0.01, 0.3, -0.3, 0.999, 1.0, 1.7, -1.7, 9.5, 10.5, -40.0, 1e6])
    across = np.stack([np.repeat(off, 4), np.tile(t[:4], len(off))], axis=1)              # (offset, along)
    along = np.stack([np.zeros(60, dtype=np.float32), t], axis=1)
    rows = np.vstack([along, across])
    if kind == "vertical line":
        rows = rows + np.float32([0.5, 0.0])
    elif kind == "horizontal line":
        rows = rows[:, ::-1] + np.float32([0.0, 0.25])
    else:
        rows = rows + np.float32([0.25, 0.5])
    Q = np.vstack([rows.astype(np.float32), P[::7], S.FAR_ROWS])
    m, c = 10, 10
    core2, _, tree = H.ref_fit(P, m, c)
    M = S.synthetic_model(len(P), 100, rng, points=P)
    for core2_, tree_ in ((core2, tree), (M.core2, M)):
        model = model_from(P, core2_, tree_, m, c, ONES)
        want = H.ref_assign(Q.astype(np.float64), P, core2_, m, tree_)
        for search in (2, 1):
            ppk_option("dbscan_search", search)
            got = assign(model, Q)
            assert np.array_equal(got, want), (search, np.flatnonzero(got != want)[:8])
    assert len(np.unique(want)) >= 4


def test_the_default_search_switches_to_the_grid_at_1024_points(ppk_option):
    ppk_option("dbscan_search", 0)
    m = 10
    far = S.FAR_ROWS[:1]
    for n, counted in ((1023, 0), (1024, 1)):
        M = S.synthetic_model(n, 50, np.random.default_rng(n))
        G = S.grid_of(M.points)
        _, _, is_all, dk2, safe = S.first_square(G, far[0].astype(np.float64), m)
        assert not is_all and not dk2 < 1.1 * safe * safe and S.regrown_square_is_all(G, dk2)   # the grid would count it
        model = model_from(M.points, M.core2, M, m, m, ONES)
        before = rows_scanned(model)
        got = assign(model, far)
        assert rows_scanned(model) - before == counted, n
        assert np.array_equal(got, H.ref_assign(far.astype(np.float64), M.points, M.core2, m, M))


@pytest.mark.parametrize("search", [1, 2])
def test_row_counts_that_fill_no_wave_or_workgroup(search, ppk_option):
    from poppunk_amd import _lib
    ppk_option("dbscan_search", search)
    m = 10
    M = S.synthetic_model(1200, 60, np.random.default_rng(12))
    model = model_from(M.points, M.core2, M, m, m, ONES)
    Q = np.random.default_rng(13).uniform(-0.1, 1.1, (257, 2)).astype(np.float32)
    want = H.ref_assign(Q.astype(np.float64), M.points, M.core2, m, M)
    for n_rows in (0, 1, 3, 5, 255, 257):
        guard = torch.full((n_rows + 8,), -7, dtype=torch.int32, device="cuda")          # nothing past the rows is written
        lab = guard[:n_rows]
        t = torch.from_numpy(Q[:n_rows].copy()).cuda()
        _lib.check(_lib.lib().ppk_dbscan_assign_dev(C.c_void_p(t.data_ptr()), n_rows, model.handle(0),
                                                    C.c_void_p(lab.data_ptr()), None), "ppk_dbscan_assign_dev")
        torch.cuda.synchronize()
        assert np.array_equal(lab.cpu().numpy(), want[:n_rows]), n_rows
        assert np.all(guard[n_rows:].cpu().numpy() == -7), n_rows
        assert np.array_equal(assign(model, Q[:n_rows]), want[:n_rows]), n_rows
    # no rows: no edges and no error
    none = torch.empty((0, 2), dtype=torch.float32, device="cuda")
    e = model.edges_dev(none)
    assert tuple(e.shape) == (0, 2)
    ne = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().ppk_dbscan_edges_dev(None, 0, 0, model.handle(0), 0, None, 0, C.c_void_p(ne.data_ptr()), None),
               "ppk_dbscan_edges_dev")
    torch.cuda.synchronize()
    assert int(ne.item()) == 0
