"""GPU tests of the shapes of ppk_network.hip that tests/test_gpu_network.py and tests/test_gpu_betweenness.py never reach
(DESIGN.md 3.7 and 3.8): offsets up to 1022, rows longer than a workgroup pass, union batches that race for one link,
labels at empty offsets, the first of several bad edges, key-width and scatter-chunk boundaries; Brandes items of
several sources, more components than the plan has threads, rows longer than a wave, components at the boundaries
between the three paths, values before the first edge and a sweep whose component order reshuffles.

Every graph and reference comes from tests/network_model.py; tests/test_network_shapes_host.py proves on the CPU that
each graph reaches the branch it was designed for.  Counts are compared with array_equal, every element.  Betweenness
is compared with an exact (integer / Fraction) Brandes or a closed form at DESIGN.md 3.8's bar,
|got - want| <= max(1e-12 |want|, 1e-15); values that are exactly 0 or 1 must be equal.  Each betweenness test prints its
worst ratio to the bar (-s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import network_model as nm  # noqa: E402
from poppunk_amd import engine  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def sweep(i, j, o, n, n_off, stride=1, labels_at=None):
    """stats (and labels) as numpy; stride 2 reads the two columns of an [m, 2] tensor in place"""
    if stride == 2:
        e = dev(np.stack([i, j], axis=1))
        i_t, j_t = e[:, 0], e[:, 1]
    else:
        i_t, j_t = dev(i), dev(j)
    stats, lab = engine.network_sweep_dev(i_t, j_t, dev(o), n, n_off, labels_at=labels_at)
    return stats.cpu().numpy(), (lab.cpu().numpy() if lab is not None else None)


# ---- counts ------------------------------------------------------------------------------------------------------------
def test_offsets_up_to_1022():
    i, j, o, n, n_off = nm.case_offsets_up_to_1022()
    want = nm.sweep_counts(i, j, o, n, n_off)
    for stride in (1, 2):
        got, _ = sweep(i, j, o, n, n_off, stride)
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]


def test_hub_rows_longer_than_a_workgroup(ppk_option):
    i, j, o, n, n_off = nm.case_hub()
    want = nm.sweep_counts(i, j, o, n, n_off)
    first, _ = sweep(i, j, o, n, n_off)
    assert np.array_equal(first, want), np.flatnonzero((first != want).any(axis=1))[:8]
    for w in (2, 64, 250):
        ppk_option("net_window", w)
        got, _ = sweep(i, j, o, n, n_off)
        assert np.array_equal(got, first), w
        assert np.array_equal(got, want), w


def test_triangle_counted_at_its_largest_offset():
    i, j, o, n, patterns = nm.triangle_orderings()
    got, _ = sweep(i, j, o, n, 3)
    # by hand: the largest offset of a pattern is 0 for 1 of the 13, 1 for 6, 2 for 6; of the 39 pairs of edges that
    # share a vertex, the larger offset is 0 for 6, 1 for 21, 2 for 12
    assert got[:, 2].tolist() == [1, 7, 13]
    assert got[:, 3].tolist() == [6, 27, 39]
    tri = np.cumsum(np.bincount([max(p) for p in patterns], minlength=3))
    wed = np.cumsum(np.bincount([max(p[a], p[b]) for p in patterns for a, b in ((0, 1), (0, 2), (1, 2))], minlength=3))
    assert got[:, 2].tolist() == tri.tolist() and got[:, 3].tolist() == wed.tolist()
    assert np.array_equal(got, nm.sweep_counts(i, j, o, n, 3))


@pytest.mark.parametrize("a,b,bridges", [(150, 150, 4000), (40, 40, 1600)])
def test_many_edges_one_link(a, b, bridges):
    i, j, o, n, n_off = nm.case_bridges(a, b, bridges)
    want = nm.sweep_counts(i, j, o, n, n_off)
    assert want[:, 1].tolist() == [2, 1]
    for call in range(3):                            # a plain repeat: the same stats every time
        for at in (0, 1):
            got, lab = sweep(i, j, o, n, n_off, labels_at=at)
            assert np.array_equal(got, want), (call, at)
            nc, want_lab = nm.labels(i, j, o, n, at)
            assert np.array_equal(lab, want_lab), (call, at)
            assert got[at, 1] == nc


def test_labels_at_offsets_without_edges():
    n, n_off = 400, 9
    i, j, o = nm.random_graph(9, n, 0.004, (3, 4, 7))
    want = nm.sweep_counts(i, j, o, n, n_off)
    # before the first edge: all singletons
    got, lab = sweep(i, j, o, n, n_off, labels_at=0)
    assert np.array_equal(got, want)
    assert np.array_equal(lab, np.arange(n))
    # an empty offset in the middle (5, 6), the empty ones before the first edge, and the last one: the graph before
    for at in (2, 5, 6, 8):
        got, lab = sweep(i, j, o, n, n_off, labels_at=at)
        assert np.array_equal(got, want)
        nc, want_lab = nm.labels(i, j, o, n, at)
        assert np.array_equal(lab, want_lab), at
        assert got[at, 1] == nc
    _, at4 = sweep(i, j, o, n, n_off, labels_at=4)
    _, at6 = sweep(i, j, o, n, n_off, labels_at=6)
    assert np.array_equal(at4, at6) and want[4, 1] > want[7, 1]


@pytest.mark.parametrize("what,size", [("n", 2), ("n", 3), ("n", 256), ("n", 257), ("n", 512), ("n", 513), ("n", 1024),
                                       ("n", 1025), ("m", 1), ("m", 4095), ("m", 4096), ("m", 4097)])
def test_vertex_and_edge_counts_at_width_boundaries(what, size):
    """n around the powers of two where the sort keys gain a bit, with the edge (n-2, n-1) at the last offset and vertex 0
    isolated; m around one scatter chunk (4096 edges) on 300 vertices; stride 1 and 2"""
    n = size if what == "n" else 300
    i, j, o = nm.width_boundary_graph(n) if what == "n" else nm.random_edges(size, n, size, range(5))
    want = nm.sweep_counts(i, j, o, n, 5)
    assert what == "n" or want[-1, 0] == size
    want_lab = nm.labels(i, j, o, n, 4)[1]
    for stride in (1, 2):
        got, lab = sweep(i, j, o, n, 5, stride, labels_at=4)
        assert np.array_equal(got, want), stride
        assert np.array_equal(lab, want_lab), stride
        if what == "n":
            assert lab[n - 2] == lab[n - 1]
            assert n == 2 or (lab[0] == 0 and (lab[1:] != 0).all())          # vertex 0 is isolated


def test_first_of_several_bad_edges_is_named():
    n, n_off, m = 300, 5, 4200
    i, j, o = nm.random_edges(42, n, m, range(n_off))
    want = nm.sweep_counts(i, j, o, n, n_off)

    def spoil(at):
        """at: {edge index: kind}"""
        bi, bj, bo = i.copy(), j.copy(), o.copy()
        for k, kind in at.items():
            if kind == "id":
                bj[k] = n
            elif kind == "loop":
                bj[k] = bi[k]
            else:
                bo[k] = n_off
        return bi, bj, bo

    cases = [({7: "id", 300: "loop", 4100: "offset"}, "edge 7 ", "vertex id out of range"),
             ({7: "loop", 300: "offset", 4100: "id"}, "edge 7 ", "self-loop"),
             ({7: "offset", 300: "id", 4100: "loop"}, "edge 7 ", "offset index out of range"),
             ({300: "offset", 4100: "id", 4199: "loop"}, "edge 300 ", "offset index out of range"),
             ({0: "loop"}, "edge 0 ", "self-loop"), ({0: "id"}, "edge 0 ", "vertex id out of range"),
             ({m - 1: "offset"}, "edge %d " % (m - 1), "offset index out of range"),
             ({m - 1: "id"}, "edge %d " % (m - 1), "vertex id out of range")]
    for at, name, why in cases:
        bi, bj, bo = spoil(at)
        for stride in (1, 2):
            with pytest.raises(RuntimeError) as err:
                sweep(bi, bj, bo, n, n_off, stride)
            assert name in str(err.value) and why in str(err.value), (at, stride, str(err.value))
            got, _ = sweep(i, j, o, n, n_off, stride)            # the next good call is unharmed
            assert np.array_equal(got, want), (at, stride)
    with pytest.raises(RuntimeError) as err:
        bi, bj, bo = spoil(cases[0][0])
        engine.network_summary_dev(dev(bi), dev(bj), dev(bo), n, n_off)
    assert "edge 7 " in str(err.value) and "vertex id out of range" in str(err.value)


# ---- betweenness -------------------------------------------------------------------------------------------------------
def ratio_to_bar(got, want):
    """the worst |got - want| / max(1e-12 |want|, 1e-15); values the reference gives as exactly 0 or 1 must be equal"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    exact = (want == 0.0) | (want == 1.0)
    assert np.array_equal(got[exact], want[exact]), np.abs(got[exact] - want[exact]).max()
    if not got.size:
        return 0.0
    return float((np.abs(got - want) / np.maximum(1e-12 * np.abs(want), 1e-15)).max())


class Worst:
    """the worst ratio to the bar of one test, printed when it is asserted"""

    def __init__(self, name):
        self.name, self.ratio = name, 0.0

    def values(self, got, want):
        self.ratio = max(self.ratio, ratio_to_bar(got.cpu().numpy(), want))

    def done(self):
        print("%s: worst |got - exact| / bar = %.3g" % (self.name, self.ratio))
        assert self.ratio <= 1.0, self.ratio


def check_graph(worst, e, n, want, summary):
    """one graph through network_summary_graph_dev: every value, both means, the count, and the stats bit for bit"""
    stats, bt, scored, values = engine.network_summary_graph_dev(dev(e), n, values=True)
    worst.values(values, want)
    worst.values(bt, np.array(nm.means(summary)))
    assert int(scored) == len(summary)
    ref, _ = engine.network_stats_dev(dev(e), n)
    assert torch.equal(stats, ref)
    return values.cpu().numpy()


@pytest.mark.parametrize("lds_max", [0, 3])
def test_items_of_several_sources(lds_max, ppk_option):
    ppk_option("bt_small_max", 0)
    ppk_option("bt_lds_max", lds_max)                # 0: state in LDS; 3: the global slab
    e, n = nm.case_multi_source()
    want, summary = nm.exact(nm.case_multi_source)
    worst = Worst("items_of_several_sources[lds_max=%d]" % lds_max)
    check_graph(worst, e, n, want, summary)
    worst.done()


@pytest.mark.parametrize("small_max", [64, 0])
@pytest.mark.parametrize("k", [256, 257, 600])
def test_more_components_than_plan_threads(k, small_max, ppk_option):
    ppk_option("bt_small_max", small_max)            # 64: every component one wave; 0: every one 256-thread items
    e, n = nm.case_many(k)
    want, summary = nm.exact(nm.case_many, k)
    assert len(summary) == k
    worst = Worst("more_components_than_plan_threads[%d, small_max=%d]" % (k, small_max))
    check_graph(worst, e, n, want, summary)
    worst.done()


@pytest.mark.parametrize("lds_max", [0, 3])
def test_rows_longer_than_a_wave(lds_max, ppk_option):
    ppk_option("bt_small_max", 0)
    ppk_option("bt_lds_max", lds_max)
    worst = Worst("rows_longer_than_a_wave[lds_max=%d]" % lds_max)
    e, n, exact = nm.case_star()
    want = np.array([float(x) for x in exact])
    got = check_graph(worst, e, n, want, [(max(exact), 301)])
    assert got.max() == 1.0 and (got == 1.0).sum() == 1 and (got == 0.0).sum() == n - 1      # the centre, the leaves
    e, n = nm.case_hub_component()
    check_graph(worst, e, n, *nm.exact(nm.case_hub_component))
    worst.done()


def test_components_at_the_path_boundaries(ppk_option):
    worst = Worst("components_at_the_path_boundaries")
    ppk_option("bt_small_max", 256)
    e, n, closed = nm.case_small_cap()
    want, summary = nm.exact(nm.case_small_cap)
    want = np.array([float(x) if x is not None else want[v] for v, x in enumerate(closed)])   # the paths: closed form
    check_graph(worst, e, n, want, summary)
    ppk_option("bt_small_max", 64)
    ppk_option("bt_lds_max", 100)
    e, n = nm.case_path_boundaries()
    check_graph(worst, e, n, *nm.exact(nm.case_path_boundaries))
    worst.done()


def test_values_before_the_first_edge():
    e, o, n, n_off = nm.case_before_first_edge()
    exact = nm.exact_sweep(nm.case_before_first_edge)
    worst = Worst("values_before_the_first_edge")
    i_t, j_t, o_t = dev(e[:, 0]), dev(e[:, 1]), dev(o)
    ref, _ = engine.network_sweep_dev(i_t, j_t, o_t, n, n_off)
    for at in (0, 1):
        stats, bt, scored, values = engine.network_summary_dev(i_t, j_t, o_t, n, n_off, values_at=at)
        assert torch.equal(stats, ref)
        assert torch.all(values == 0).item() and values.shape[0] == n
        assert bt[:2].tolist() == [[0.0, 0.0]] * 2 and scored[:2].tolist() == [0, 0]
        for t in range(n_off):
            worst.values(bt[t], np.array(nm.means(exact[t][1])))
            assert int(scored[t]) == len(exact[t][1]), t
    _, _, _, values = engine.network_summary_dev(i_t, j_t, o_t, n, n_off, values_at=2)
    worst.values(values, exact[2][0])
    worst.done()


def test_sweep_where_component_order_changes():
    e, o, n, n_off = nm.case_reorder()
    exact = nm.exact_sweep(nm.case_reorder)
    worst = Worst("sweep_where_component_order_changes")
    i_t, j_t, o_t = dev(e[:, 0]), dev(e[:, 1]), dev(o)
    ref, _ = engine.network_sweep_dev(i_t, j_t, o_t, n, n_off)
    assert np.array_equal(ref.cpu().numpy(), nm.sweep_counts(e[:, 0], e[:, 1], o, n, n_off))
    for at in (5, 10):
        stats, bt, scored, values = engine.network_summary_dev(i_t, j_t, o_t, n, n_off, values_at=at)
        assert torch.equal(stats, ref)
        worst.values(values, exact[at][0])
        for t in range(n_off):
            worst.values(bt[t], np.array(nm.means(exact[t][1])))
            assert int(scored[t]) == len(exact[t][1]), t
    worst.done()
