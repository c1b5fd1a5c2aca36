"""GPU tests of the network sweep (ppk_network_sweep_dev): per-offset edges, components, triangles
and connected triples against a numpy / scipy brute force, component labels against scipy, growNetwork and the
chained sweep -> scores path against the reference-derived golden (tests/golden/network_sweep.npz), and the
argument errors."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, distfile, engine, refine  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "network_sweep.npz")
DEV = "cuda:0"


def brute(i, j, o, n, n_off):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    A = np.zeros((n, n))
    out = np.zeros((n_off, 4), dtype=np.int64)
    row = np.array([0, n, 0, 0])
    for t in range(n_off):
        sel = o == t
        if sel.any():
            A[i[sel], j[sel]] = 1
            A[j[sel], i[sel]] = 1
            deg = A.sum(1).astype(np.int64)
            row = np.array([int(A.sum()) // 2, connected_components(csr_matrix(A), directed=False)[0],
                            int(round(((A @ A) * A).sum() / 6)), int((deg * (deg - 1) // 2).sum())])
        out[t] = row
    return out


def random_graph(rng, n, p, n_off, used_offsets):
    ii, jj = np.triu_indices(n, 1)
    keep = rng.random(ii.size) < p
    i, j = ii[keep], jj[keep]
    o = rng.choice(used_offsets, size=i.size)
    swap = rng.random(i.size) < 0.5
    i, j = np.where(swap, j, i), np.where(swap, i, j)
    perm = rng.permutation(i.size)
    return i[perm].astype(np.int64), j[perm].astype(np.int64), o[perm].astype(np.int64)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


@pytest.mark.parametrize("n,p,n_off", [(301, 0.02, 40), (301, 0.3, 40), (129, 0.5, 1), (77, 0.2, 1023),
                                       (515, 0.05, 40)])
def test_counts_equal_brute_force(n, p, n_off):
    rng = np.random.default_rng(n * 7 + n_off)
    used = np.sort(rng.choice(n_off, size=max(1, (2 * n_off) // 3), replace=False)) if n_off > 1 else np.array([0])
    used = used[:60]                                   # many empty batches at 1023
    i, j, o = random_graph(rng, n, p, n_off, used)
    want = brute(i, j, o, n, n_off)
    stats, lab = engine.network_sweep_dev(dev(i), dev(j), dev(o), n, n_off)
    assert np.array_equal(stats.cpu().numpy(), want)
    # an [m, 2] edge list read in place (stride 2)
    e = dev(np.stack([i, j], axis=1))
    stats2, _ = engine.network_sweep_dev(e[:, 0], e[:, 1], dev(o), n, n_off)
    assert np.array_equal(stats2.cpu().numpy(), want)
    # host arrays
    hs, _ = refine.network_sweep(i, j, o, n, n_off)
    assert np.array_equal(hs, want)


def test_forced_windows_change_nothing():
    rng = np.random.default_rng(5)
    n, n_off = 700, 40
    i, j, o = random_graph(rng, n, 0.08, n_off, np.arange(0, n_off, 2))
    want, _ = engine.network_sweep_dev(dev(i), dev(j), dev(o), n, n_off)
    old = _lib.get_option("net_window")
    try:
        for w in (2, 64, 250):
            _lib.set_option("net_window", w)
            got, _ = engine.network_sweep_dev(dev(i), dev(j), dev(o), n, n_off)
            assert torch.equal(got, want), w
    finally:
        _lib.set_option("net_window", old)
    assert np.array_equal(want.cpu().numpy(), brute(i, j, o, n, n_off))


def test_labels_equal_scipy():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(11)
    n, n_off = 1000, 12
    i, j, o = random_graph(rng, n, 0.0015, n_off, np.arange(n_off))
    for at in (0, 5, n_off - 1):
        stats, lab = engine.network_sweep_dev(dev(i), dev(j), dev(o), n, n_off, labels_at=at)
        sel = o <= at
        g = coo_matrix((np.ones(sel.sum()), (i[sel], j[sel])), shape=(n, n))
        nc, want = connected_components(g, directed=False)
        assert np.array_equal(lab.cpu().numpy(), want)
        assert int(stats[at, 1]) == nc


def test_empty_and_single_offset():
    e = torch.zeros((0, 2), dtype=torch.int64, device=DEV)
    stats, lab = engine.network_stats_dev(e, 17, labels=True)
    assert stats.tolist() == [0, 17, 0, 0]
    assert lab.tolist() == list(range(17))
    z = torch.zeros(0, dtype=torch.int64, device=DEV)
    stats, _ = engine.network_sweep_dev(z, z, z, 9, 5)
    assert stats.tolist() == [[0, 9, 0, 0]] * 5


def test_grow_network_reproduces_golden():
    z = np.load(GOLDEN)
    for case in (str(c) for c in z["cases"]):
        n = int(z[case + "_n"])
        stats, _ = refine.network_sweep(z[case + "_i"], z[case + "_j"], z[case + "_idx"], n, int(z[case + "_n_off"]))
        assert np.array_equal(stats, z[case + "_stats"]), case
        got = np.array(refine.growNetwork(["s%d" % k for k in range(n)], z[case + "_i"], z[case + "_j"],
                                          z[case + "_idx"], list(range(int(z[case + "_n_off"])))), dtype=np.float64)
        want = z[case + "_scores"]
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), case
        np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-12, atol=0)
        for t, m in zip(z[case + "_present"], z[case + "_metrics"]):
            metrics, _ = refine.summary_from_stats(stats[t], n)
            assert metrics[0] == m[0] and metrics[1] == m[1]
            assert (np.isnan(metrics[2]) and np.isnan(m[2])) or metrics[2] == m[2]


def test_chained_sweep_scores_reproduce_golden():
    z = np.load(GOLDEN)
    x0, y0, x1, y1 = z["sweep1d_line"]
    stats, scores = engine.refine_sweep_scores_dev(dev(z["sweep1d_dist"]), z["sweep1d_offsets"], 2, x0, y0, x1, y1)
    assert np.array_equal(stats.cpu().numpy(), z["sweep1d_stats"])
    want = z["sweep1d_scores"]
    got = np.array(scores)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-12, atol=0)
    stats, scores = engine.refine_sweep_scores_2d_dev(dev(z["sweep2d_dist"]), z["sweep2d_xmax"], float(z["sweep2d_ymax"]))
    assert np.array_equal(stats.cpu().numpy(), z["sweep2d_stats"])
    np.testing.assert_allclose(scores, z["sweep2d_scores"], rtol=1e-12, atol=0)


def test_chained_sweep_on_rand363_equals_host_path():
    from oracle import oracle
    d = np.load(os.path.join(HERE, "golden", "boundary_refine.npz"))["rand363"]
    x1, y1 = float(np.median(d[:, 0])), float(np.median(d[:, 1]))
    offs = np.linspace(0.0, float(np.hypot(x1, y1)), 40)
    stats, scores = engine.refine_sweep_scores_dev(dev(d), offs, 2, 0.0, 0.0, x1, y1)
    i, j, o = oracle.threshold_iterate_1d(d, offs, 2, 0.0, 0.0, x1, y1)
    want = brute(i, j, o, 363, 40)
    assert np.array_equal(stats.cpu().numpy(), want)
    host = refine.grow_scores(want, 363)
    assert np.array_equal(np.isnan(scores), np.isnan(host))
    np.testing.assert_allclose(np.array(scores)[~np.isnan(host)], np.array(host)[~np.isnan(host)], rtol=0, atol=0)


def test_fused_edges_to_labels_equal_clusters_from_edges():
    from poppunk_amd import synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(300, kmers, cluster_size=30)
    tbl = synth.random_match_table(kmers)
    db = engine.SketchDB(sk, 16, 14, device=0)
    try:
        dist, _ = engine.dist(db, None, kmers, tbl)
        x_max, y_max = synth.boundary_for_quantile(dist.cpu().numpy(), 0.05)
        edges, _ = engine.dist_edges(db, None, kmers, tbl, slope=2, x_max=x_max, y_max=y_max)
    finally:
        db.close()
    assert edges.shape[0] > 0
    stats, lab = engine.network_stats_dev(edges, 300, labels=True)
    nc, want = distfile.clusters_from_edges(300, edges.cpu().numpy())
    assert int(stats[1]) == nc and int(stats[0]) == edges.shape[0]
    assert np.array_equal(lab.cpu().numpy(), want)


def test_errors_name_an_edge_and_the_next_call_succeeds():
    lib = _lib.lib()
    i = dev(np.array([0, 1, 2, 3], dtype=np.int64))
    j = dev(np.array([1, 2, 3, 4], dtype=np.int64))
    o = dev(np.array([0, 1, 1, 2], dtype=np.int64))
    st = torch.zeros((8, 4), dtype=torch.int64, device=DEV)
    lab = torch.zeros(8, dtype=torch.int32, device=DEV)

    def call(i_t, j_t, o_t, n, n_off, labels_at=-1, stride=1):
        return lib.ppk_network_sweep_dev(i_t.data_ptr(), j_t.data_ptr(), stride,
                                         o_t.data_ptr() if o_t is not None else None, i_t.shape[0], n, n_off,
                                         labels_at, st.data_ptr(), lab.data_ptr(), None)

    bad_j = dev(np.array([1, 2, 9, 4], dtype=np.int64))
    cases = [((i, bad_j, o, 5, 3), b"edge 2"), ((i, dev(np.array([1, 2, 2, 4], dtype=np.int64)), o, 5, 3), b"self-loop"),
             ((i, j, dev(np.array([0, 1, 3, 2], dtype=np.int64)), 5, 3), b"offset"),
             ((dev(np.array([0, -1, 2, 3], dtype=np.int64)), j, o, 5, 3), b"edge 1"),
             ((i, j, o, 5, 0), b"n_off"), ((i, j, o, 5, 1024), b"n_off"), ((i, j, o, 1 << 31, 3), b"n_vertices"),
             ((i, j, None, 5, 3), b"n_off"), ((i, j, o, 5, 3, 3), b"labels_at")]
    for args, msg in cases:
        assert call(*args) == _lib.ERR_ARG, msg
        assert msg in lib.ppk_last_error(), (msg, lib.ppk_last_error())
        assert call(i, j, o, 5, 3, 1) == _lib.OK
        torch.cuda.synchronize()
        assert st[:3].tolist() == [[1, 4, 0, 0], [3, 2, 0, 2], [4, 1, 0, 3]]
        assert lab[:5].tolist() == [0, 0, 0, 0, 1]
    with pytest.raises(RuntimeError, match="ppk_network_sweep_dev"):
        engine.network_sweep_dev(i, bad_j, o, 5, 3)
