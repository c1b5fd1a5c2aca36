"""Minimum spanning forests and model edge weights on the device (ppk_mst_dev, ppk_edge_weights_dev):
against a Python Kruskal under the same total order, scipy, numpy's process_weights and the reference's
generate_minimum_spanning_tree (tests/golden/mst.npz)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, network, sparse_mst, synth  # noqa: E402
from mst_shapes import kruskal, multigraph, scipy_labels  # noqa: E402,F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mst.npz")
DEV = "cuda:0"


def run(e, w, n, labels=True):
    et = torch.as_tensor(e, device=DEV).contiguous()
    wt = torch.as_tensor(w, dtype=torch.float32, device=DEV)
    tree, n_comp, lab = engine.mst_dev(et, wt, n, labels=labels)
    return tree.cpu().numpy(), n_comp, (lab.cpu().numpy() if labels else None)


@pytest.mark.parametrize("seed,n,n_comp,n_edges,levels", [(0, 50, 3, 200, 4), (1, 300, 6, 3000, 3),
                                                           (2, 1000, 10, 4000, 20), (3, 5000, 25, 40000, 6),
                                                           (4, 5000, 2, 20000, 2)])
def test_matches_kruskal_and_scipy_labels(seed, n, n_comp, n_edges, levels):
    rng = np.random.default_rng(seed)
    e, w = multigraph(rng, n, n_comp, n_edges, levels)
    tree, comps, lab = run(e, w, n)
    want = kruskal(e, n, w)
    assert np.array_equal(tree, want)
    sc, sl = scipy_labels(e, n)
    assert comps == sc and tree.size == n - sc
    assert np.array_equal(lab, sl)


def test_permuted_and_swapped_input_gives_the_same_edge_set_and_repeats_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 3000
    e, w = multigraph(rng, n, 8, 30000, 5)
    tree, _, lab = run(e, w, n)
    again, _, lab2 = run(e, w, n)
    assert np.array_equal(tree, again) and np.array_equal(lab, lab2)

    def edge_set(ee, ww, t):
        x = ee[t]
        return sorted(zip(x.min(axis=1).tolist(), x.max(axis=1).tolist(), (ww[t] + np.float32(0)).tolist()))
    p = rng.permutation(len(e))
    e2 = e[p].copy()
    sw = rng.random(len(e)) < 0.5
    e2[sw] = e2[sw][:, ::-1]
    t2, _, lab3 = run(e2, w[p], n)
    # the same (min, max, w) set: the tie among parallel copies of one pair picks a copy, not a different pair
    assert edge_set(e, w, tree) == edge_set(e2, w[p], t2)
    assert np.array_equal(lab, lab3)


def test_strided_pair_and_host_twin():
    rng = np.random.default_rng(6)
    e, w = multigraph(rng, 400, 4, 2000, 7)
    et = torch.as_tensor(e, device=DEV).contiguous()
    wt = torch.as_tensor(w, device=DEV)
    a, _, _ = engine.mst_dev((et[:, 0], et[:, 1]), wt, 400)
    b, _, _ = engine.mst_dev((et[:, 0].contiguous(), et[:, 1].contiguous()), wt, 400)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(network.device_mst(e, 400, w), a.cpu().numpy())


def test_errors_and_empty_inputs():
    et = torch.tensor([[0, 1], [1, 2]], dtype=torch.int64, device=DEV)
    ok = torch.tensor([1.0, 2.0], device=DEV)
    with pytest.raises(RuntimeError, match="edge 1 .*out of range"):
        engine.mst_dev(et, ok, 2)
    with pytest.raises(RuntimeError, match="edge 0 .*self-loop"):
        engine.mst_dev(torch.tensor([[1, 1], [0, 1]], dtype=torch.int64, device=DEV), ok, 3)
    with pytest.raises(RuntimeError, match="edge 1 .*NaN"):
        engine.mst_dev(et, torch.tensor([1.0, float("nan")], device=DEV), 3)
    with pytest.raises(RuntimeError, match="edge 0 .*infinite"):
        engine.mst_dev(et, torch.tensor([float("inf"), 1.0], device=DEV), 3)
    with pytest.raises(TypeError):
        engine.mst_dev(et, ok.double(), 3)
    lib = _lib.lib()
    assert lib.ppk_mst_dev(None, None, 1, None, 0, 1 << 31, None, None, None, None) == _lib.ERR_ARG
    empty = torch.zeros((0, 2), dtype=torch.int64, device=DEV)
    tree, comps, lab = engine.mst_dev(empty, torch.zeros(0, device=DEV), 7, labels=True)
    assert tree.numel() == 0 and comps == 7 and lab.cpu().tolist() == list(range(7))
    tree, comps, lab = engine.mst_dev(empty, torch.zeros(0, device=DEV), 1, labels=True)
    assert tree.numel() == 0 and comps == 1 and lab.cpu().tolist() == [0]


# ---- edge weights ----------------------------------------------------------------------------------------------

def process_weights(rows, kind):
    """PopPUNK/network.py:646-674 restated: float32 rows in, the list's values as float32."""
    if kind == "euclidean":
        return np.linalg.norm(rows, axis=1)
    return rows[:, 0] if kind == "core" else rows[:, 1]


@pytest.mark.parametrize("kind", ["core", "accessory", "euclidean"])
@pytest.mark.parametrize("self_comp,off", [(True, 0), (True, 7), (False, 0), (False, 3)])
def test_edge_weights_match_process_weights(kind, self_comp, off):
    rng = np.random.default_rng(9)
    n_ref, n_qry = 90, 40
    rows = n_ref * (n_ref - 1) // 2 if self_comp else n_ref * n_qry
    dist = (rng.random((rows, 2)) * np.array([0.05, 0.6])).astype(np.float32)
    dist[::17] = 0.0
    assign = (rng.random(rows) < 0.3).astype(np.int32) * 2 - 1             # within_label -1
    dist_t = torch.as_tensor(dist, device=DEV)
    a_t = torch.as_tensor(assign, device=DEV)
    edges = engine.generate_tuples_dev(a_t, -1, self_comparison=self_comp, num_ref=0 if self_comp else n_ref,
                                       int_offset=off)
    got = engine.edge_weights_dev(dist_t, edges, kind, n_ref=0 if self_comp else n_ref, int_offset=off)
    want = process_weights(dist[assign == -1], kind).astype(np.float32)
    assert got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    sw = torch.stack([edges[:, 1], edges[:, 0]], dim=1).contiguous()        # either orientation
    got2 = engine.edge_weights_dev(dist_t, sw, kind, n_ref=0 if self_comp else n_ref, int_offset=off)
    assert torch.equal(got, got2)


def test_edge_weights_errors():
    dist_t = torch.rand((45, 2), device=DEV)                               # n = 10
    with pytest.raises(RuntimeError, match="edge 1 .*no row"):
        engine.edge_weights_dev(dist_t, torch.tensor([[0, 1], [3, 10]], device=DEV))
    with pytest.raises(RuntimeError, match="edge 0 .*no row"):
        engine.edge_weights_dev(dist_t, torch.tensor([[2, 2]], device=DEV))
    with pytest.raises(RuntimeError, match="edge 0 .*no row"):                # both ends refs: no non-self row
        engine.edge_weights_dev(dist_t[:40], torch.tensor([[0, 1]], device=DEV), n_ref=8)
    with pytest.raises(TypeError):
        engine.edge_weights_dev(dist_t.double(), torch.tensor([[0, 1]], device=DEV))
    with pytest.raises(TypeError):
        engine.edge_weights_dev(dist_t, torch.tensor([[0, 1]], dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        engine.edge_weights_dev(dist_t.t().contiguous().t(), torch.tensor([[0, 1]], device=DEV))
    with pytest.raises(ValueError):
        engine.edge_weights_dev(dist_t, torch.tensor([[0, 1]], device=DEV), "jaccard")


# ---- generate_minimum_spanning_tree against the reference --------------------------------------------------------

def golden_cases():
    return [str(c) for c in np.load(GOLDEN)["cases"]]


@pytest.mark.parametrize("case", golden_cases())
@pytest.mark.parametrize("on_device", [True, False])
def test_generate_minimum_spanning_tree_golden(case, on_device):
    z = np.load(GOLDEN)
    e, n, w = z[case + "_edges"], int(z[case + "_n"]), z[case + "_weights"]
    want_e, want_w = z[case + "_out_edges"], z[case + "_out_weights"]
    n_comp = int(z[case + "_n_components"])
    G = (torch.as_tensor(e, device=DEV), n, torch.as_tensor(w.astype(np.float32), device=DEV)) if on_device \
        else (e, n, w.astype(np.float32))
    got_e, got_n, got_w = network.generate_minimum_spanning_tree(G)
    k = n - n_comp
    assert got_n == n and np.array_equal(got_e[:k], want_e[:k]) and np.array_equal(got_w, want_w)
    links = got_e[k:]
    assert links.shape[0] == max(n_comp - 1, 0)
    seeds = set(z[case + "_seeds"].tolist())
    assert set(links.ravel().tolist()) <= seeds
    if n_comp == 2:                                         # the only case where the seed link is unique
        assert sorted(links[0].tolist()) == sorted(want_e[k].tolist())
    _, lab = scipy_labels(got_e, n)
    assert lab.max() == 0                                   # every component joined


def test_generate_network_dense_and_sparse():
    rng = np.random.default_rng(12)
    n = 120
    rows = n * (n - 1) // 2
    dist = (rng.random((rows, 2)) * np.array([0.05, 0.6])).astype(np.float32)
    dist_t = torch.as_tensor(dist, device=DEV)
    from poppunk_amd.models import RefineBoundary
    model = RefineBoundary.from_threshold(0.01)
    edges, gn, w = network.generate_network_from_distances("dense", model, core_distMat=dist_t,
                                                           combined_seq=["s%d" % k for k in range(n)],
                                                           distance_type="euclidean")
    assign = model.assign(dist)
    want_e = np.array(np.nonzero(np.triu(np.ones((n, n)), 1))).T[assign == -1]
    assert gn == n and np.array_equal(edges.cpu().numpy(), want_e)
    assert np.array_equal(w.cpu().numpy(), np.linalg.norm(dist[assign == -1], axis=1))
    with pytest.raises(NotImplementedError):
        network.generate_network_from_distances("dense", model, core_distMat=dist_t, previous_mst="x")
    from scipy.sparse import coo_matrix
    pick = rng.random(rows) < 0.05
    ij = np.array(np.nonzero(np.triu(np.ones((n, n)), 1))).T[pick]
    sp = coo_matrix((dist[pick, 0], (ij[:, 0], ij[:, 1])), shape=(n, n))
    ge, gn, gw = network.generate_network_from_distances("sparse", None, sparse_mat=sp, rlist=list(range(n)))
    tree = kruskal(ij, n, dist[pick, 0])
    k = tree.size
    assert np.array_equal(ge[:k], ij[tree]) and np.array_equal(gw[:k], dist[pick, 0][tree].astype(np.float64))
    t_e, _, t_w = sparse_mst.generate_mst_from_sparse_input(
        (torch.as_tensor(ij[:, 0], device=DEV), torch.as_tensor(ij[:, 1], device=DEV),
         torch.as_tensor(dist[pick, 0], device=DEV)), list(range(n)))
    assert np.array_equal(t_e, ge) and np.array_equal(t_w, gw)


# ---- scale: bench.py's sweep graph and a 100 000-genome kNN graph against scipy -------------------------------------

def scipy_tree_weights(e, w, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    t = minimum_spanning_tree(coo_matrix((w.astype(np.float64), (e[:, 0], e[:, 1])), shape=(n, n)).tocsr())
    return np.sort(t.data)


def check_against_scipy(e_t, w_t, n):
    tree, comps, lab = engine.mst_dev(e_t, w_t, n, labels=True)
    e, w = e_t.cpu().numpy(), w_t.cpu().numpy()
    pos = w > 0
    assert pos.all()
    sc, sl = scipy_labels(e, n)
    assert comps == sc and tree.numel() == n - sc and np.array_equal(lab.cpu().numpy(), sl)
    got = np.sort(w[tree.cpu().numpy()].astype(np.float64))
    assert np.array_equal(got, scipy_tree_weights(e, w, n))
    again, _, _ = engine.mst_dev(e_t, w_t, n)
    assert torch.equal(tree, again)


def test_scale_sweep_graph_core_weights():
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(10_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    xs = (dist / dist.amax(dim=0)).contiguous()
    sample = xs[::20].cpu().numpy()
    m0, m1 = np.quantile(sample, 0.01, axis=0), np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, _ = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    e_t = torch.stack([i, j], dim=1).contiguous()
    w_t = engine.edge_weights_dev(dist, e_t, "core")
    keep = w_t > 0
    check_against_scipy(e_t[keep].contiguous(), w_t[keep].contiguous(), 10_000)


def test_scale_knn_graph():
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(100_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    gi, gj, gd = engine.knn_from_sketches(db, kmers, tbl, 10)
    db.close()
    keep = gd > 0
    e_t = torch.stack([gi[keep], gj[keep]], dim=1).contiguous()
    check_against_scipy(e_t, gd[keep].to(torch.float32).contiguous(), 100_000)
