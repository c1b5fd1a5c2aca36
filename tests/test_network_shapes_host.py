"""CPU checks of tests/network_model.py (no device): its references against independent ones, and every designed case
of tests/test_gpu_network_shapes.py against the condition it was designed for, read from the graph itself and from the
restated plan, so that a change of a generator or of a kernel constant cannot quietly move a case off its branch."""
import importlib.util
import os
import time
from fractions import Fraction

import numpy as np
import pytest

import network_model as nm

HERE = os.path.dirname(os.path.abspath(__file__))


def up_degrees(i, j, n):
    """|N+(v)|: the neighbours of v with a higher id"""
    return np.bincount(np.minimum(i, j), minlength=n)


def degrees(e, n):
    return np.bincount(np.asarray(e).reshape(-1), minlength=n)


# ---- the references ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,n_off,used", [(60, 0.2, 1, (0,)), (97, 0.1, 7, (0, 2, 3, 6)), (120, 0.3, 40, range(0, 40, 3)),
                                            (77, 0.2, 1023, None), (120, 0.05, 1023, nm.HIGH_OFFSETS)])
def test_sweep_counts_equal_the_dense_brute_force(n, p, n_off, used):
    if used is None:
        used = np.random.default_rng(n).choice(1023, size=40, replace=False).tolist() + [1022]
    i, j, o = nm.random_graph(n + n_off, n, p, list(used))
    assert o.max() == max(used)
    assert np.array_equal(nm.sweep_counts(i, j, o, n, n_off), nm.brute_counts(i, j, o, n, n_off))


def test_sweep_counts_of_the_triangle_orderings_equal_the_hand_count():
    i, j, o, n, patterns = nm.triangle_orderings()
    want = nm.sweep_counts(i, j, o, n, 3)
    assert want[:, 0].tolist() == [18, 33, 39]
    assert want[:, 2].tolist() == [1, 7, 13] and want[:, 3].tolist() == [6, 27, 39]
    assert np.array_equal(want, nm.brute_counts(i, j, o, n, 3))
    assert len(set(patterns)) == 13 and not nm.has_repeated_pair(i, j)


def load_float_brandes():
    """the float Python Brandes and the clustered generator of tests/test_gpu_betweenness.py (its torch import skips
    this test where torch is absent)"""
    pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("gpu_betweenness_ref", os.path.join(HERE, "test_gpu_betweenness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_brandes_exact_equals_the_float_brandes_on_the_clustered_graph():
    ref = load_float_brandes()
    e, n = ref.clustered_graph(np.random.default_rng(1))
    t0 = time.perf_counter()
    got, summary = nm.brandes_exact(e, n)
    print("brandes_exact, clustered graph of %d vertices: %.2f s" % (n, time.perf_counter() - t0))
    want, want_summary = ref.brandes(e, n)
    assert np.abs(got - want).max() <= 1e-12
    assert sorted(s for _, s in summary) == sorted(s for _, s in want_summary)
    np.testing.assert_allclose(nm.means(summary), ref.means(want_summary), rtol=1e-12, atol=1e-15)
    assert np.abs(nm.brandes_float(e, n) - got).max() <= 1e-12
    assert np.abs(nm.brandes_float(e, n, reverse_rows=True) - got).max() <= 1e-12


@pytest.mark.parametrize("pairs,size,want", [
    (nm.star(8), 9, nm.star_values(8)), (nm.star(300), 301, nm.star_values(300)), (nm.star(2), 3, nm.star_values(2)),
    (nm.path(4), 4, nm.path_values(4)), (nm.path(37), 37, nm.path_values(37)), (nm.path(3), 3, nm.path_values(3)),
    (nm.clique(7), 7, nm.clique_values(7)), (nm.cycle(4), 4, nm.cycle_values(4)), (nm.cycle(9), 9, nm.cycle_values(9)),
    (nm.cycle(12), 12, nm.cycle_values(12)), (nm.bipartite(3, 5), 8, nm.bipartite_values(3, 5)),
    (nm.bipartite(1, 6), 7, nm.bipartite_values(1, 6)), (nm.bipartite(4, 4), 8, nm.bipartite_values(4, 4))])
def test_brandes_exact_equals_every_closed_form(pairs, size, want):
    got, summary = nm.brandes_exact(np.array(pairs, dtype=np.int64), size, fractions=True)
    assert got == want                                # Fraction equality
    assert all(isinstance(x, Fraction) for x in got)
    assert summary == ([(max(want), size)] if size > 3 else [])
    assert nm.path_values(4)[1] == Fraction(2, 3) and nm.cycle_values(4)[0] == Fraction(1, 6)


def test_plan_on_hand_worked_components():
    # W = 10 * (18 + 10) + 2000 * (6000 + 2000) = 16 000 280; target = 15 625.27...; costs 28 and 8000
    got = nm.plan([(2000, 6000), (10, 18), (4, 6)], small_max=4, lds_max=1000)
    assert (got["K"], got["K_big"], got["K_glob"]) == (3, 2, 1)
    assert got["s"] == [2, 10, 4] and got["items"] == [1000, 1, 1]
    # nothing above small_max: W = 0, target 1, every component one item of all its sources
    got = nm.plan([(10, 18), (4, 6)], small_max=64, lds_max=0)
    assert (got["K"], got["K_big"], got["K_glob"]) == (2, 0, 0) and got["s"] == [10, 4] and got["items"] == [1, 1]
    # small_max is clamped to the one-wave kernel's capacity
    assert nm.plan([(257, 512)], small_max=1000, lds_max=0)["K_big"] == 1


# ---- the designed cases: counts ----------------------------------------------------------------------------------------------
def test_case_offsets_reach_the_top_of_the_field():
    i, j, o, n, n_off = nm.case_offsets_up_to_1022()
    assert n_off == 1023 and not nm.has_repeated_pair(i, j)
    for t in nm.HIGH_OFFSETS:
        assert (o == t).sum() > 0, t
    assert (o >= 512).sum() > i.size // 3
    want = nm.sweep_counts(i, j, o, n, n_off)
    # triangles and triples appear at 1022, and at an offset >= 512 whose low 9 bits name an unused offset: a histogram
    # that dropped the top bit would change rows here
    assert want[1022, 2] > want[1021, 2] and want[1022, 3] > want[1021, 3]
    assert any(t >= 512 and (t & 511) not in o and want[t, 2] > want[t - 1, 2] for t in np.unique(o))


def test_case_hub_rows_are_longer_than_a_workgroup():
    i, j, o, n, n_off = nm.case_hub()
    assert n == 700 and not nm.has_repeated_pair(i, j)
    up = up_degrees(i, j, n)
    assert up[0] >= 600 and up[0] > 2 * 256           # the four 256-strided loops take a third pass
    assert up[1] >= 200 and up[1] > 3 * 64            # the 64-strided walk of N+(v) takes a fourth step
    sel = (np.minimum(i, j) == 0) & (np.maximum(i, j) == 1)
    assert sel.sum() == 1                             # ... for v = 1 in N+(0)
    assert np.unique(o).size == 12
    t0 = time.perf_counter()
    want = nm.sweep_counts(i, j, o, n, n_off)
    dt = time.perf_counter() - t0
    print("sweep_counts, hub graph of %d edges: %.2f s" % (i.size, dt))
    assert dt < 20.0 and want[-1, 2] > 5000


@pytest.mark.parametrize("a,b,bridges", [(150, 150, 4000), (40, 40, 1600)])
def test_case_bridges_make_one_link(a, b, bridges):
    i, j, o, n, n_off = nm.case_bridges(a, b, bridges)
    assert not nm.has_repeated_pair(i, j) and (o == 1).sum() == bridges and (o == 0).sum() == n - 2
    want = nm.sweep_counts(i, j, o, n, n_off)
    assert want[:, 1].tolist() == [2, 1]              # thousands of edges race for one link
    nc, lab = nm.labels(i, j, o, n, 0)
    assert nc == 2
    sides = lab[i[o == 1]] != lab[j[o == 1]]
    assert sides.all()                                # every bridge joins the same two sets


def test_case_width_boundary_graphs():
    for n in (2, 3, 256, 257, 512, 513, 1024, 1025):
        i, j, o = nm.width_boundary_graph(n)
        assert not nm.has_repeated_pair(i, j) and i.size >= 1
        last = (np.minimum(i, j) == n - 2) & (np.maximum(i, j) == n - 1)
        assert last.sum() == 1 and o[last][0] == 4
        if n > 2:
            assert 0 not in i and 0 not in j
    for m in (1, 4095, 4096, 4097):
        i, j, o = nm.random_edges(m, 300, m, range(5))
        assert i.size == m and not nm.has_repeated_pair(i, j)


# ---- the designed cases: betweenness -----------------------------------------------------------------------------------------
def timed_exact(case, *args):
    t0 = time.perf_counter()
    out = nm.exact(case, *args)
    dt = time.perf_counter() - t0
    print("brandes_exact, %s%r: %.2f s" % (case.__name__, args, dt))
    assert dt < 30.0                                  # (a few seconds where measured; the bound is generous)
    return out


def test_case_multi_source_items():
    e, n = nm.case_multi_source()
    assert not nm.has_repeated_pair(e)
    sa = nm.sizes_adj(e, n)
    assert sa[0][0] == 120 and 1800 <= sum(nc for nc, _ in sa) <= 2400
    for lds_max in (0, 3):
        p = nm.plan(sa, small_max=0, lds_max=lds_max)
        assert p["K"] == p["K_big"] == 301 and p["K_glob"] == (301 if lds_max else 0)
        multi = [(nc, s) for (nc, _), s in zip(sa, p["s"]) if 1 < s < nc]
        assert len(multi) >= 50                                   # items that reuse their state across sources
        assert sum(1 for nc, s in multi if nc % s) >= 20          # ... with a short last item
        assert any(it > 1 and s > 1 for s, it in zip(p["s"], p["items"]))     # bt_reduce sums several partials
    timed_exact(nm.case_multi_source)


@pytest.mark.parametrize("k", [256, 257, 600])
def test_case_more_components_than_plan_threads(k):
    e, n = nm.case_many(k)
    assert not nm.has_repeated_pair(e)
    sa = nm.sizes_adj(e, n)
    sizes = [nc for nc, _ in sa]
    assert len(sa) == k and set(sizes) == {4, 5, 6}
    assert max(sizes.count(x) for x in (4, 5, 6)) > k // 4        # many of equal size: the order falls to the root
    assert n > sum(sizes)                                         # and some components of <= 3 vertices
    for small_max, big in ((64, 0), (0, k)):
        p = nm.plan(sa, small_max=small_max, lds_max=0)
        assert (p["K"], p["K_big"], p["K_glob"]) == (k, big, 0)
    timed_exact(nm.case_many, k)


def test_case_rows_longer_than_a_wave():
    e, n, want = nm.case_star()
    d = degrees(e, n)
    assert d.max() == 300 > 256 and not nm.has_repeated_pair(e)
    assert sorted(want, reverse=True)[:2] == [1, 0] and None not in want
    for lds_max in (0, 3):
        p = nm.plan(nm.sizes_adj(e, n), small_max=0, lds_max=lds_max)
        assert (p["K"], p["K_big"], p["K_glob"]) == (1, 1, 1 if lds_max else 0)
    got, _ = nm.brandes_exact(e, n, fractions=True)
    assert got == want
    e, n = nm.case_hub_component()
    d = degrees(e, n)
    assert d.max() == 299 > 256 and not nm.has_repeated_pair(e)
    sa = nm.sizes_adj(e, n)
    assert sa[0][0] == 300 and 850 <= sa[0][1] // 2 <= 950 and len(sa) == 2
    timed_exact(nm.case_hub_component)


def test_case_components_at_the_path_boundaries():
    e, n, want = nm.case_small_cap()
    assert not nm.has_repeated_pair(e)
    sa = nm.sizes_adj(e, n)
    assert [nc for nc, _ in sa] == [257, 256, 256]
    assert sorted(adj // 2 for _, adj in sa) == [255, 256, 480]          # the two paths and the 16 x 16 lattice
    p = nm.plan(sa, small_max=256, lds_max=0)
    assert (p["K"], p["K_big"], p["K_glob"]) == (3, 1, 0)                # 256 is small_max, 257 is small_max + 1
    values, summary = timed_exact(nm.case_small_cap)
    closed = np.array([float(x) if x is not None else np.nan for x in want])
    assert np.isnan(closed).sum() == 256
    ok = ~np.isnan(closed)
    assert np.array_equal(values[ok], closed[ok])                        # both round the exact value once
    e, n = nm.case_path_boundaries()
    assert not nm.has_repeated_pair(e)
    sa = nm.sizes_adj(e, n)
    assert tuple(sorted(nc for nc, _ in sa)) == nm.BOUNDARY_SIZES == (64, 65, 100, 101)
    p = nm.plan(sa, small_max=64, lds_max=100)
    assert (p["K"], p["K_big"], p["K_glob"]) == (4, 3, 1)
    timed_exact(nm.case_path_boundaries)


def test_case_values_before_the_first_edge():
    e, o, n, n_off = nm.case_before_first_edge()
    assert n_off == 5 and o.min() == 2 and not nm.has_repeated_pair(e)
    assert len(nm.exact_sweep(nm.case_before_first_edge)[4][1]) >= 8
    assert nm.exact_sweep(nm.case_before_first_edge)[1][1] == []


def test_case_component_order_changes_along_the_sweep():
    e, o, n, n_off = nm.case_reorder()
    assert n_off == 12 and not nm.has_repeated_pair(e)
    assert np.unique(o).size == 12
    t0 = time.perf_counter()
    sweep = nm.exact_sweep(nm.case_reorder)
    dt = time.perf_counter() - t0
    print("brandes_exact, 12 graphs of the reordering sweep: %.2f s" % dt)
    assert dt < 30.0
    scored = [len(s) for _, s in sweep]
    assert max(scored) > scored[-1] > 0 and scored[0] < max(scored)      # components appear, then merge
    # the (size descending, smallest vertex) order: some pair of components that both persist swaps places
    swaps = 0
    for t in range(1, n_off):
        before = [c[0][0] for c in nm.components(e[o <= t - 1], n)[0]]
        after = [c[0][0] for c in nm.components(e[o <= t], n)[0]]
        both = [r for r in before if r in after]
        swaps += [r for r in after if r in both] != both
    assert swaps >= 3
