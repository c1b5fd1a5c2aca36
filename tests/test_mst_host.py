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
