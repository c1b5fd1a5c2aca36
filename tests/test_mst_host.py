"""CPU tests of generate_minimum_spanning_tree's host step (network.seed_links) against tests/golden/mst.npz, the
reference's own function run on a graph-tool stand-in (tests/golden/make_golden_mst.py), with host Kruskals as the
MST callables.  No device."""
import os

import numpy as np
import pytest

from poppunk_amd import network

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mst.npz")


def kruskal_by_weight(edges, n, weights):
    """The golden stand-in's min_spanning_tree: a stable sort on the weight alone (earlier edge wins a tie)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    parent = list(range(int(n)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    keep = []
    for k in np.argsort(np.asarray(weights, dtype=np.float64), kind="stable").tolist():
        a, b = find(int(e[k, 0])), find(int(e[k, 1]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            keep.append(k)
    return np.array(sorted(keep), dtype=np.int64)


def cases():
    z = np.load(GOLDEN)
    return [str(c) for c in z["cases"]]


@pytest.mark.parametrize("case", cases())
def test_seed_step_matches_the_reference(case):
    z = np.load(GOLDEN)
    edges, n, w = z[case + "_edges"], int(z[case + "_n"]), z[case + "_weights"]
    out_e, out_w = z[case + "_out_edges"], z[case + "_out_weights"]
    n_comp = int(z[case + "_n_components"])
    tree = network.kruskal(edges, n, w)                     # distinct weights: the forest is unique
    assert np.array_equal(tree, kruskal_by_weight(edges, n, w))
    k = n - n_comp
    assert tree.size == k
    assert np.array_equal(edges[tree], out_e[:k]) and np.array_equal(w[tree], out_w[:k])
    seeds, got_comp = network.forest_seeds(edges[tree], n)
    assert got_comp == n_comp and list(seeds) == z[case + "_seeds"].tolist()
    add, add_w = network.seed_links(edges[tree], edges, w, n, kruskal_by_weight)
    assert np.array_equal(add, out_e[k:]), "seed links differ from the reference's"
    assert add_w.size == n_comp - 1 if n_comp > 1 else add_w.size == 0
    assert np.all(out_w[k:] == 0.0)                         # appended without a weight property
    if n_comp > 1:
        assert np.all(add_w == np.max(w))                   # every link is the max_weight fallback


def test_two_components_link_is_unique_under_either_tie_rule():
    z = np.load(GOLDEN)
    edges, n, w = z["two_edges"], int(z["two_n"]), z["two_weights"]
    tree = network.kruskal(edges, n, w)
    add, _ = network.seed_links(edges[tree], edges, w, n, network.kruskal)
    assert sorted(add[0].tolist()) == sorted(z["two_out_edges"][-1].tolist())


def test_seed_to_seed_edges_of_g_are_taken_when_the_forest_does_not_span_g():
    # forest: {0-1}, {2-3}, {4}; G also joins the seeds 0 and 2 (weight 5), so seeds 0 and 2 take G's edge and seed 4,
    # with no edge at it, links to both other seeds at max_weight 9
    forest = np.array([[0, 1], [2, 3]])
    g = np.array([[0, 1], [2, 3], [2, 0], [1, 4]])
    gw = np.array([1.0, 2.0, 5.0, 9.0])
    seeds, n_comp = network.forest_seeds(forest, 5)
    assert list(seeds) == [0, 2, 4] and n_comp == 3
    conn = []

    def record(e, k, w):
        conn.append((e.copy(), w.copy()))
        return network.kruskal(e, k, w)
    add, add_w = network.seed_links(forest, g, gw, 5, record)
    e, w = conn[0]
    assert e.tolist() == [[0, 2], [2, 0], [4, 0], [4, 2]] and w.tolist() == [5.0, 5.0, 9.0, 9.0]
    assert add.tolist() == [[0, 2], [4, 0]] and add_w.tolist() == [5.0, 9.0]


def test_seed_graph_can_stay_disconnected():
    # seeds 0 and 2 joined by G's edge, 4 and 6 likewise: every seed has a seed edge, no fallback, two seed components
    forest = np.zeros((0, 2), dtype=np.int64)
    g = np.array([[0, 2], [4, 6]])
    add, _ = network.seed_links(forest, g, np.array([1.0, 2.0]), 8, network.kruskal)
    # seeds 1, 3, 5 and 7 have no edge at all: they fall back to every other seed, which joins everything
    assert add.shape[0] == 7
    add, _ = network.seed_links(forest, g, np.array([1.0, 2.0]), 7, network.kruskal)
    assert add.shape[0] == 6
    forest = np.array([[0, 1], [2, 3], [4, 5], [6, 7]])
    add, _ = network.seed_links(forest, np.array([[0, 2], [4, 6]]), np.array([1.0, 2.0]), 8, network.kruskal)
    assert add.tolist() == [[0, 2], [4, 6]]                 # 4 components, 2 links: the result stays disconnected


def test_no_edges_raises_as_np_max_does():
    with pytest.raises(ValueError):
        network.seed_links(np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2), dtype=np.int64), np.zeros(0), 3,
                           network.kruskal)


def test_kruskal_total_order():
    # equal weights: (min, max, index) decides; -0.0 == +0.0
    e = np.array([[1, 2], [0, 2], [2, 0], [0, 1]])
    w = np.array([0.0, -0.0, 0.0, 1.0])
    assert network.kruskal(e, 3, w).tolist() == [0, 1]


# ---- tests/mst_shapes.py: what every builder claims (tests/test_gpu_mst_shapes.py runs them on the device) -----------
import mst_shapes as S  # noqa: E402


@pytest.mark.parametrize("n,passes", [(16, 1), (200, 3), (600, 3), (10_000, 5)])
def test_two_chains_hook_into_two_deep_trees_and_join_in_round_two(n, passes):
    e, w, tree = S.two_chains(n)
    h = n // 2
    assert np.array_equal(tree, np.arange(n - 1)) and e[n - 2].tolist() == [0, h]
    got, rounds, depths = S.boruvka(e, w, n)
    assert np.array_equal(got, tree) and rounds == 2
    assert depths[0] == n - h - 1                           # the longer chain, root to far end
    # the depth needs every pass the device runs that is not there for parity alone
    need = next(p for p in range(1, 9) if 16 ** p >= depths[0])
    assert S.jump_passes(n) == passes and need in (passes, passes - 1) and need == next(
        p for p in range(1, 9) if 16 ** p >= n)
    assert np.array_equal(S.kruskal(e, n, w), tree)
    e2, w2, pos = S.shuffled(e, w, n)
    assert np.array_equal(S.kruskal(e2, n, w2), np.sort(pos[tree]))
    assert np.array_equal(S.boruvka(e2, w2, n)[0], np.sort(pos[tree]))


def test_two_chains_claims_at_140_000_vectorised():
    n = 140_000
    h = n // 2
    e, w, tree = S.two_chains(n)                            # asserts the float32 round trip itself
    assert S.jump_passes(n) == 5 and n - h - 1 > 16 ** 4
    chain, cross, chord = slice(0, n - 2), slice(n - 2, n - 2 + h), slice(n - 2 + h, None)
    assert len(e) == (n - 2) + h + (n - 4)
    for lo, hi, first in ((0, h - 1, 0), (h - 1, n - 2, h)):
        ee, ww = e[lo:hi], w[lo:hi]
        assert np.array_equal(ee[:, 0], np.arange(first, first + hi - lo)) and np.array_equal(ee[:, 1], ee[:, 0] + 1)
        # strictly heavier along the chain: at vertex k the edge to k - 1, ww[k - first - 1], is lighter than the one to
        # k + 1, ww[k - first]
        assert (np.diff(ww.astype(np.float64)) > 0).all()
    assert np.array_equal(e[cross], np.stack([np.arange(h), np.arange(h) + h], axis=1))
    assert (np.diff(w[cross].astype(np.float64)) > 0).all() and tree[-1] == n - 2
    assert w[chain].max() < w[chord].min() and w[chord].max() < w[cross].min()
    d = e[chord]
    assert np.array_equal(d[:, 1], d[:, 0] + 2) and ((d[:, 0] < h) == (d[:, 1] < h)).all()   # inside one chain


@pytest.mark.parametrize("n", [2, 4, 8, 1024, 4096])
def test_ruler_needs_ceil_log2_rounds_at_powers_of_two(n):
    e, w, tree = S.ruler(n)
    got, rounds, _ = S.boruvka(e, w, n)
    assert np.array_equal(got, tree) and np.array_equal(tree, np.arange(n - 1))
    assert rounds == S.ceil_log2(n) == n.bit_length() - 1
    assert np.array_equal(S.kruskal(e, n, w), tree)
    assert (e[n - 1:, 1] - e[n - 1:, 0] == 3).all() and (w[n - 1:] >= 64).all() and (w[:n - 1] < 64).all()


@pytest.mark.parametrize("n", [3, 5, 1025])
def test_ruler_off_a_power_of_two_pins_no_round_count(n):
    # recorded so that nobody mistakes these sizes for pins: the forest is done a round early
    e, w, tree = S.ruler(n)
    got, rounds, _ = S.boruvka(e, w, n)
    assert np.array_equal(got, tree) and rounds == S.ceil_log2(n) - 1


@pytest.mark.parametrize("n", [2, 3, 256, 257])
def test_equal_weights_builder(n):
    e, w = S.equal_weights(n, n)
    assert (w == np.float32(0.5)).all() and e.min() >= 0 and e.max() < n and (e[:, 0] != e[:, 1]).all()
    pairs = set(map(tuple, np.sort(e, axis=1).tolist()))
    for a, b in ((0, n - 1), (1, n - 1), (n - 2, n - 1), (n // 2, n // 2 + 1)):
        assert (a, b) in pairs or a == b or b >= n
    if n >= 16:
        assert 3 <= np.setdiff1d(np.arange(n), e.ravel()).size <= n // 16   # a few isolated
        assert ((e[:, 0] < e[:, 1]).mean() > 0.3) and ((e[:, 0] > e[:, 1]).mean() > 0.3)
        assert len(e) - len(pairs) > 0.05 * len(e)                      # parallel copies
    tree = S.kruskal(e, n, w)
    assert np.array_equal(S.boruvka(e, w, n)[0], tree)
    assert tree.size == n - S.scipy_labels(e, n)[0]


def test_weight_range_builder_holds_every_listed_value_and_ties():
    e, w = S.weight_range(300, 300)
    vals = S.weight_levels(np.random.default_rng(0))
    assert len(vals) == 26 and (np.isfinite(vals)).all()
    assert set(vals[:14].view(np.uint32).tolist()) <= set(w.view(np.uint32).tolist())
    assert (w < 0).any() and np.abs(w).max() == np.float32(3.4028235e38)
    assert np.abs(w[w != 0]).min() == np.float32(1.4e-45)
    assert (np.signbit(w) & (w == 0)).any() and (~np.signbit(w) & (w == 0)).any()
    tree = S.kruskal(e, 300, w)
    assert np.array_equal(S.boruvka(e, w, 300)[0], tree) and np.array_equal(network.kruskal(e, 300, w), tree)
    # the two zeros must share a key: under the order of the raw bit patterns (-0.0 before +0.0) the forest differs,
    # and so it does under the order of the magnitudes alone and of the bit patterns read as integers
    def by_rank(key):
        return S.kruskal(e, 300, np.unique(key, return_inverse=True)[1].astype(np.float32))
    u = w.view(np.uint32)
    assert np.array_equal(by_rank(w.astype(np.float64) + 0.0), tree)
    raw = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))
    assert not np.array_equal(by_rank(raw), tree)
    assert not np.array_equal(by_rank(np.abs(w)), tree) and not np.array_equal(by_rank(u), tree)


def test_known_forest_is_its_own_answer():
    n = 3000
    e, w, tree, labels = S.known_forest(n, 5, 2, 12_000, 7)
    assert len(e) == 12_000 and tree.size == n - 7
    assert np.array_equal(S.kruskal(e, n, w), tree)
    sc, sl = S.scipy_labels(e, n)
    assert sc == 7 and np.array_equal(labels, sl)
    assert len(np.unique(w[tree])) > 32 and tree.size > 10 * len(np.unique(w[tree]))    # many ties


def test_known_forest_beyond_one_grid_claims():
    n, m = (1 << 20) + 3, (1 << 22) + 1000
    e, w, tree, labels = S.known_forest(n, 5, 2, m, 11)
    assert len(e) == m and tree.size == 1_048_572 and labels.max() == 6
    chord = np.ones(m, dtype=bool)
    chord[tree] = False
    assert w[tree].max() < 1.0 and w[chord].min() >= 2.0                 # every chord heavier than every forest edge
    assert np.array_equal(labels[e[:, 0]], labels[e[:, 1]])              # every edge inside one component
    assert (e[:, 0] != e[:, 1]).all() and e.min() >= 0 and e.max() < n
    # the forest edges alone give the same 7 components: they span every run
    sc, sl = S.scipy_labels(e[tree], n)
    assert sc == 7 and np.array_equal(sl, labels)
    assert np.bincount(labels).min() == 1 and (np.bincount(labels) == 1).sum() == 2     # the two isolated vertices


def test_euclid_rows_references_agree_bit_for_bit():
    x = S.euclid_rows(363, 3)
    assert x.shape == (65_703, 2) and x.dtype == np.float32
    want = S.euclid_expected(x)
    with np.errstate(over="ignore", under="ignore"):
        norm = np.linalg.norm(x, axis=1)
    assert norm.dtype == np.float32 and np.array_equal(norm.view(np.uint32), want.view(np.uint32))
    tiny = np.float32(1.17549435e-38)
    assert np.isinf(want).sum() >= 1 and np.isfinite(x).all()
    assert ((x != 0) & (np.abs(x) < tiny)).any(axis=1).sum() >= 1        # a subnormal coordinate
    assert (x == 0).all(axis=1).sum() >= 1 and (want == 0).sum() >= 1
    assert (np.signbit(x) & (x == 0)).any() and (x == 0).any(axis=1).mean() > 0.01
    with np.errstate(over="ignore", under="ignore"):
        sq = x[:, 0] * x[:, 0]
        ss = sq + x[:, 1] * x[:, 1]
    assert ((sq != 0) & (sq < tiny)).any() and ((sq == 0) & (x[:, 0] != 0)).any()   # squares that underflow
    assert ((ss != 0) & (ss < tiny)).any() and np.isinf(ss).any()        # a subnormal sum (its root is normal), inf
    p = S.all_pairs(363)
    assert len(p) == len(x) and (p[:, 0] < p[:, 1]).all() and len(set(map(tuple, p.tolist()))) == len(p)
