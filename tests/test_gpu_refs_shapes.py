"""GPU tests of the component shapes of ppk_refs.hip: every size at which the code takes another
path -- 1 and 2 (the unconditional lowest vertex), 3 (the first wave-pruned size), 63 / 64 / 65 (the wave and
workgroup switch, a full word, a second word with one bit), 127 / 128 / 129 (the word edges again) -- as cliques,
paths and random graphs of density 0.5, several of them side by side so that more than one wave and workgroup runs;
and the global-scratch route of the large kernels against their LDS route.  Device against the restatement of
tests/refs_model.py, bit for bit, plus the property checker."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import refs_model as rm  # noqa: E402
from test_gpu_refs import agree, on_device  # noqa: E402

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129)
KINDS = {"clique": lambda k: rm.clique(k), "path": lambda k: rm.path(k),
         "random": lambda k: rm.random_graph(k, 0.5, 100 + k) if k > 1 else []}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("size", SIZES)
def test_one_component(size, kind):
    r, _, c = agree(KINDS[kind](size), size)
    assert c["components"] == 1 and r[0] == 1
    if kind == "clique":
        assert c["references"] == 1


def test_triangle_and_three_path():
    r, _, c = agree(rm.clique(3), 3)
    assert r.tolist() == [1, 0, 0] and c["cliques_removed"] == 1
    r, _, c = agree(rm.path(3), 3)                  # {0, 1} then the leftover {2}; the repair adds 1
    assert r.tolist() == [1, 1, 1] and c["cliques_removed"] == 2 and c["added_by_repair"] == 1


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_size_side_by_side(kind):
    e, n = rm.shifted([(KINDS[kind](k), k) for k in SIZES + SIZES[::-1]])
    rng = np.random.default_rng(4)
    e = e[rng.permutation(len(e))]
    _, _, c = agree(e, n)
    assert c["components"] == 2 * len(SIZES)
    existing = (rng.random(n) < 0.05).astype(np.uint8)
    agree(e, n, existing)


def test_pair_whose_higher_vertex_is_an_existing_reference():
    existing = np.array([0, 1, 0, 0, 1], dtype=np.uint8)
    r, _, c = agree([(0, 1), (3, 4)], 5, existing)
    assert r.tolist() == [1, 1, 1, 1, 1] and c["from_small"] == 3


def test_interleaved_components_keep_the_index_order():
    """components whose vertices alternate: the local index is the rank within the component, not an offset"""
    k = 70
    a = [(2 * x, 2 * y) for x, y in rm.random_graph(k, 0.5, 1)]
    b = [(2 * x + 1, 2 * y + 1) for x, y in rm.path(k)]
    agree(a + b, 2 * k)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_global_route_equals_the_lds_route(kind, ppk_option):
    e, n = rm.shifted([(KINDS[kind](129), 129), (rm.dumbbell(70, 4)[0], 144), (KINDS[kind](65), 65)])
    lds = on_device(e, n)
    ppk_option("refs_lds_bits", 64)
    glob = agree(e, n)
    assert np.array_equal(lds[0], glob[0]) and np.array_equal(lds[1], glob[1]) and lds[2] == glob[2]
    assert glob[2]["components_repaired"] >= 1       # the BFS ran on the global route too
