"""GPU tests of the shapes of ppk_mst.hip that tests/test_gpu_mst.py never reaches: hook forests that
need every pointer-jumping pass and the odd pass count, paths that need every one of the ceil(log2 n) rounds, pair keys
at 2^k and 2^k + 1 vertices and wider than 32 bits, weights over the whole finite float32 range, more vertices and edges
than one grid covers, the smallest and most degenerate inputs, and the Euclidean weight of rows from subnormal to
overflowing.

The inputs come from tests/mst_shapes.py, and tests/test_mst_host.py proves on the CPU that each is what it claims to
be.  The references are the Kruskal of tests/mst_shapes.py under the contract's total order, scipy's component labels,
the builders' own answers and numpy's float32 arithmetic.  Every comparison is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mst_shapes as S  # noqa: E402
from poppunk_amd import engine, network  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"


def run(e, w, n, labels=True):
    et = torch.as_tensor(np.ascontiguousarray(e, dtype=np.int64).reshape(-1, 2), device=DEV)
    wt = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32), device=DEV)
    tree, n_comp, lab = engine.mst_dev(et, wt, n, labels=labels)
    return tree.cpu().numpy(), n_comp, (lab.cpu().numpy() if labels else None)


def differ(got, want):
    """The head of both sides' symmetric difference, for the assertion message."""
    return np.setdiff1d(got, want)[:6], np.setdiff1d(want, got)[:6]


# ---- jump passes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 200, 600, 10_000, 140_000])
def test_two_chains_need_every_jump_pass(n):
    # passes 1, 3 (made odd from 2), 3, 5 (made odd from 4), 5; first-round depth 7, 99, 299, 4 999, 69 999
    e, w, tree = S.two_chains(n)
    got, comps, lab = run(e, w, n)
    assert np.array_equal(got, tree), differ(got, tree)
    assert comps == 1 and not lab.any()
    e2, w2, pos = S.shuffled(e, w, n)
    want = np.sort(pos[tree])
    got, comps, lab = run(e2, w2, n)
    assert np.array_equal(got, want), differ(got, want)
    assert comps == 1 and not lab.any()


# ---- rounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 1024, 65_536])
def test_ruler_needs_every_round(n):
    e, w, tree = S.ruler(n)
    got, comps, lab = run(e, w, n)
    assert got.size == n - 1 and comps == 1 and not lab.any()
    assert np.array_equal(got, tree), differ(got, tree)                   # every path edge, no chord
    if n == 1024:
        assert np.array_equal(network.device_mst(e, n, w), tree)          # the host form
        et = torch.as_tensor(e, device=DEV)
        pair, _, _ = engine.mst_dev((et[:, 0], et[:, 1]), torch.as_tensor(w, device=DEV), n)
        assert np.array_equal(pair.cpu().numpy(), tree)
        pair, _, _ = engine.mst_dev((et[:, 0].contiguous(), et[:, 1].contiguous()), torch.as_tensor(w, device=DEV), n)
        assert np.array_equal(pair.cpu().numpy(), tree)


# ---- key bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 256, 257, 65_536, 65_537])
def test_equal_weights_at_powers_of_two(n):
    # bits = 1, 2, 8, 9, 16, 17: at 2^k the top bit of the key's min field is in use, at 65 537 the key is 34 bits wide
    e, w = S.equal_weights(n, n)
    got, comps, lab = run(e, w, n)
    want = S.kruskal(e, n, w)
    assert np.array_equal(got, want), differ(got, want)
    sc, sl = S.scipy_labels(e, n)
    assert comps == sc and got.size == n - sc and np.array_equal(lab, sl)


# ---- weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 3000])
def test_weight_order_over_the_float_range(n):
    e, w = S.weight_range(n, n)
    got, comps, lab = run(e, w, n)
    want = S.kruskal(e, n, w)                # float64 order of float32 values + 0.0: the contract's order
    assert np.array_equal(got, want), (differ(got, want), w[differ(got, want)[0]], w[differ(got, want)[1]])
    sc, sl = S.scipy_labels(e, n)
    assert comps == sc and np.array_equal(lab, sl)


# ---- grid strides ----------------------------------------------------------------------------------------------------
def test_known_forest_beyond_one_grid():
    # n > 1 048 576: every vertex loop strides; m > 4 194 304: every edge loop strides, mst_min_kernel's among them
    n, m = (1 << 20) + 3, (1 << 22) + 1000
    e, w, tree, labels = S.known_forest(n, 5, 2, m, 11)
    et, wt = torch.as_tensor(e, device=DEV), torch.as_tensor(w, device=DEV)
    got, comps, lab = engine.mst_dev(et, wt, n, labels=True)
    assert comps == 7
    assert np.array_equal(got.cpu().numpy(), tree), differ(got.cpu().numpy(), tree)
    assert np.array_equal(lab.cpu().numpy(), labels)
    bare, comps2, none = engine.mst_dev(et, wt, n, labels=False)
    assert none is None and comps2 == 7 and torch.equal(bare, got)
    again, _, lab2 = engine.mst_dev(et, wt, n, labels=True)
    assert torch.equal(again, got) and torch.equal(lab2, lab)


# ---- tiny and degenerate ---------------------------------------------------------------------------------------------
def test_tiny_and_degenerate():
    got, comps, lab = run(np.zeros((0, 2)), np.zeros(0), 0)
    assert got.size == 0 and comps == 0 and lab.size == 0
    got, comps, lab = run([[0, 1], [1, 0]], [0.25, 0.25], 2)
    assert got.tolist() == [0] and comps == 1 and lab.tolist() == [0, 0]
    got, comps, lab = run([[1, 0], [0, 1]], [0.25, 0.25], 2)
    assert got.tolist() == [0] and comps == 1 and lab.tolist() == [0, 0]
    e = np.tile(np.array([[0, 1], [1, 0]]), (500, 1))
    got, comps, lab = run(e, np.full(1000, -3.5), 5)
    assert got.tolist() == [0] and comps == 4 and lab.tolist() == [0, 0, 1, 2, 3]
    got, comps, lab = run(e + 3, np.full(1000, -3.5), 5)
    assert got.tolist() == [0] and comps == 4 and lab.tolist() == [0, 1, 2, 3, 3]
    # only the last two of 4 097 vertices: the lightest copy, then the first of its weight, -0.0 tying with +0.0
    n = 4097
    e = np.array([[n - 1, n - 2], [n - 2, n - 1], [n - 1, n - 2], [n - 2, n - 1], [n - 1, n - 2]])
    got, comps, lab = run(e, [1.0, 0.0, -0.0, 0.0, 2.0], n)
    assert got.tolist() == [1] and comps == n - 1
    assert np.array_equal(lab, np.minimum(np.arange(n), n - 2))
    assert np.array_equal(S.kruskal(e, n, [1.0, 0.0, -0.0, 0.0, 2.0]), [1])


# ---- edge weights ----------------------------------------------------------------------------------------------------
def test_euclidean_weights_over_the_float_range():
    x = S.euclid_rows(363, 3)
    want = S.euclid_expected(x)
    dist_t = torch.as_tensor(x, device=DEV)
    pairs = torch.as_tensor(S.all_pairs(363), device=DEV)               # every row used once, in row order
    got = engine.edge_weights_dev(dist_t, pairs, "euclidean").cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, x[bad[:6]], got[bad[:6]], want[bad[:6]])
    for col, kind in enumerate(("core", "accessory")):
        got = engine.edge_weights_dev(dist_t, pairs, kind).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), x[:, col].view(np.uint32))
