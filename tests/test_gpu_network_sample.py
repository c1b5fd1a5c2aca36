"""GPU tests of the sampled-source betweenness and the whole-graph values (ppk_network_summary_sampled*):
the boundary of the sampling rule, every launch path with a source list, a row longer than a wave under sampling, a
sweep whose components merge, determinism, the whole-graph flag, the argument errors and the Python mirrors.

Every graph and reference comes from tests/network_sample_model.py (exact integer / Fraction Brandes over the model's
source lists); tests/test_network_sample_host.py proves on the CPU that each graph reaches the branch it names.  The
bar is DESIGN.md 3.8's own, |got - want| <= max(1e-12 |want|, 1e-15); values that are exactly 0 or 1 must be equal.  Each
test prints its worst ratio to the bar (-s)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import network_model as nm  # noqa: E402
import network_sample_model as sm  # noqa: E402
from poppunk_amd import _lib, assign, engine, models, network, refine  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


class Worst:
    def __init__(self, name):
        self.name, self.ratio = name, 0.0

    def values(self, got, want):
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        self.ratio = max(self.ratio, sm.bar_ratio(got, want))

    def done(self):
        print("%s: worst |got - exact| / bar = %.3g" % (self.name, self.ratio))
        assert self.ratio <= 1.0, self.ratio


def sampled(e, n, k, seed=0, whole=False):
    """one graph through the sampled call -> (stats, bt, scored, values) as numpy"""
    out = engine.network_summary_sampled_graph_dev(dev(e), n, values=True, sources=k, seed=seed, whole_graph=whole)
    return tuple(x.cpu().numpy() for x in out)


def check_graph(worst, e, n, k, seed, want):
    """every value, both means, the count, and the stats bit for bit"""
    values_want, summary, _ = want
    stats, bt, scored, values = sampled(e, n, k, seed)
    worst.values(values, values_want)
    worst.values(bt, np.array(nm.means(summary)))
    assert int(scored) == len(summary)
    ref, _ = engine.network_stats_dev(dev(e), n)
    assert np.array_equal(stats, ref.cpu().numpy())
    return values


# ---- the boundary of the rule --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sm.RULE_SIZES)
def test_boundary_of_the_rule(size):
    e, n = sm.case_rule_boundary(size)
    worst = Worst("boundary_of_the_rule[%d]" % size)
    values = check_graph(worst, e, n, sm.RULE_K, 0, sm.exact(sm.case_rule_boundary, sm.RULE_K, 0, False, size))
    if size <= sm.RULE_K:
        _, bt, _, exact_values = refine.network_summary(e[:, 0], e[:, 1], None, n, 1, values_at=0)
        assert np.array_equal(values, exact_values)
        assert np.array_equal(sampled(e, n, sm.RULE_K)[1], bt[0])
    else:
        exact_values = engine.network_summary_graph_dev(dev(e), n, values=True)[3].cpu().numpy()
        assert not np.array_equal(values, exact_values)
    worst.done()


# ---- each launch path with a source list ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_max", [0, 100])
def test_items_of_several_sources_from_a_list(lds_max, ppk_option):
    ppk_option("bt_small_max", 8)
    ppk_option("bt_lds_max", lds_max)                # 0: state in LDS; 100: the 120-vertex component on the global slab
    e, n = nm.case_multi_source()
    worst = Worst("items_of_several_sources_from_a_list[lds_max=%d]" % lds_max)
    check_graph(worst, e, n, 50, 0, sm.exact(nm.case_multi_source, 50, 0))
    worst.done()


@pytest.mark.parametrize("lds_max", [0, 3])
def test_items_of_two_listed_sources_and_a_short_last_item(lds_max, ppk_option):
    ppk_option("bt_small_max", 5)                    # exactly the sampled components (n_c > 5) are 256-thread items:
    ppk_option("bt_lds_max", lds_max)                # 2 + 2 + 1 sources of their lists; 3: every one on the global slab
    e, n = nm.case_multi_source()
    worst = Worst("items_of_two_listed_sources_and_a_short_last_item[lds_max=%d]" % lds_max)
    check_graph(worst, e, n, 5, 0, sm.exact(nm.case_multi_source, 5, 0))
    worst.done()


def test_one_wave_path_with_a_list():
    e, n = nm.case_multi_source()
    worst = Worst("one_wave_path_with_a_list")
    check_graph(worst, e, n, 5, 0, sm.exact(nm.case_multi_source, 5, 0))
    worst.done()


@pytest.mark.parametrize("k", [64, 65])
def test_around_the_one_wave_cap(k):
    e, n = sm.case_cap()
    worst = Worst("around_the_one_wave_cap[k=%d]" % k)
    check_graph(worst, e, n, k, 0, sm.exact(sm.case_cap, k, 0))
    worst.done()


# ---- a row longer than a wave under sampling ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["centre_in", "centre_out"])
def test_star_under_sampling(which, ppk_option):
    ppk_option("bt_small_max", 0)
    e, n, centre = sm.case_star()
    seed = sm.star_seeds()[0 if which == "centre_in" else 1]
    want = sm.exact(sm.case_star, sm.STAR_K, seed)
    sample = next(iter(want[2].values()))
    assert (centre in sample) == (which == "centre_in") and len(sample) == sm.STAR_K
    worst = Worst("star_under_sampling[%s]" % which)
    values = check_graph(worst, e, n, sm.STAR_K, seed, want)
    leaves_in_sample = [v for v in sample if v != centre]
    # a sampled leaf is on no path from the other sources; every other leaf neither: the leaves are all 0
    assert np.count_nonzero(values) == 1 and values[centre] > 0 and all(values[v] == 0.0 for v in leaves_in_sample)
    worst.done()


# ---- a sweep in which components merge -----------------------------------------------------------------------------------------
def test_sweep_with_merging_components():
    e, o, n, n_off = nm.case_reorder()
    want = sm.exact_sweep(nm.case_reorder, 6, 0)
    i_t, j_t, o_t = dev(e[:, 0]), dev(e[:, 1]), dev(o)
    ref, _ = engine.network_sweep_dev(i_t, j_t, o_t, n, n_off)
    worst = Worst("sweep_with_merging_components")
    stats, bt, scored, values = engine.network_summary_sampled_dev(i_t, j_t, o_t, n, n_off, values_at=7, sources=6)
    assert torch.equal(stats, ref)
    for t in range(n_off):
        worst.values(bt[t], np.array(nm.means(want[t][1])))
        assert int(scored[t]) == len(want[t][1]), t
    worst.values(values, want[7][0])
    worst.done()


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call_and_for_any_edge_order(ppk_option):
    ppk_option("bt_small_max", 8)
    e, n = nm.case_multi_source()
    first = sampled(e, n, 50, 0)
    for _ in range(2):
        again = sampled(e, n, 50, 0)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    rng = np.random.default_rng(5)
    again = sampled(e[rng.permutation(e.shape[0])][:, ::-1], n, 50, 0)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # another seed: another sample of the 120-vertex component, and its own exact values
    big = min(sm.exact(nm.case_multi_source, 50, 0)[2])
    assert sm.exact(nm.case_multi_source, 50, 0)[2][big] != sm.exact(nm.case_multi_source, 50, 1)[2][big]
    worst = Worst("second_seed")
    values = check_graph(worst, e, n, 50, 1, sm.exact(nm.case_multi_source, 50, 1))
    assert not np.array_equal(values, first[3])
    worst.done()


# ---- the whole-graph flag --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [sm.K_ALL - 1, 10])
def test_whole_graph_values(k):
    e, n, ids = sm.case_whole()
    want, summary, _ = sm.exact(sm.case_whole, k, 0, True)
    worst = Worst("whole_graph_values[k=%d]" % k)
    stats, bt, scored, values = sampled(e, n, k, 0, whole=True)
    worst.values(values, want)
    for part in (6, 7):                                     # the two 3-paths: ends 0, the middle 2 / ((n - 1)(n - 2))
        got = values[ids[part]]
        assert got[0] == 0.0 and got[2] == 0.0 and got[1] == 2.0 / (39.0 * 38.0)
    assert np.count_nonzero(values[np.concatenate([ids[p] for p in range(6)] + [ids[8]])]) == 0
    flag0 = sampled(e, n, k, 0)
    assert np.array_equal(bt, flag0[1]) and int(scored) == int(flag0[2]) == 2 and np.array_equal(stats, flag0[0])
    worst.values(bt, np.array(nm.means(summary)))
    worst.done()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_call():
    e, n, _ = sm.case_whole()
    i, j = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    stats, bt = np.zeros((1, 4), dtype=np.int64), np.zeros((1, 2))
    llp, dp = C.POINTER(C.c_longlong), C.POINTER(C.c_double)

    def call(k, flags):
        return _lib.lib().ppk_network_summary_sampled(i.ctypes.data_as(llp), j.ctypes.data_as(llp), None, i.size, n, 1, 0,
                                                      -1, stats.ctypes.data_as(llp), bt.ctypes.data_as(dp), None, None,
                                                      k, 0, flags)

    for k, flags, text in ((0, 0, "bt_sources"), (5, 2, "flag"), (5, 1 | 4, "flag")):
        assert call(k, flags) == _lib.ERR_ARG
        msg = _lib.last_error()
        assert msg.startswith("ppk_network_summary_sampled:") and text in msg, msg
    i_t, j_t = dev(i), dev(j)
    with pytest.raises(ValueError):
        engine.network_summary_sampled_dev(i_t, j_t, None, n, 1, sources=0)
    with pytest.raises(RuntimeError, match="ppk_network_summary_sampled: edge [0-9]+ .*vertex id out of range"):
        engine.network_summary_sampled_dev(i_t, j_t, None, 3, 1, sources=5)
    assert call(5, 0) == _lib.OK and int(stats[0, 0]) == e.shape[0]


# ---- the Python mirrors ------------------------------------------------------------------------------------------------------------
def test_network_summary_with_sampled_betweenness():
    e, o, n, _ = nm.case_reorder()
    _, summary, _ = sm.sampled_exact(e, n, 6, 3)
    want_bt = np.array(nm.means(summary))
    worst = Worst("network_summary_with_sampled_betweenness")
    for edges in (e, dev(e)):
        metrics, scores = network.networkSummary((edges, n), sampled_betweenness=True, betweenness_sample=6, seed=3)
        worst.values(np.array(metrics[3:5]), want_bt)
        base = network.networkSummary((edges, n), calc_betweenness=False)[1][0]
        assert scores[0] == base and scores[1] == base * (1 - metrics[3]) and scores[2] == base * (1 - metrics[4])
    exact_metrics, _ = network.networkSummary((e, n), betweenness_sample=6)      # the default ignores the sample
    assert not np.array_equal(np.array(exact_metrics[3:5]), np.array(metrics[3:5]))
    worst.done()


def test_vertex_betweenness():
    e, n, _ = sm.case_whole()
    worst = Worst("vertex_betweenness")
    for edges in (e, dev(e)):
        worst.values(network.vertex_betweenness((edges, n)), sm.whole_exact(e, n))
        worst.values(network.vertex_betweenness((edges, n), norm=False), sm.whole_exact(e, n, norm=False))
        worst.values(network.vertex_betweenness((edges, n), betweenness_sample=10, seed=4),
                     sm.sampled_exact(e, n, 10, 4, whole=True)[0])
    assert np.array_equal(network.vertex_betweenness((np.array([[0, 1]]), 2)), np.zeros(2))
    worst.done()


def test_assign_prints_the_betweenness_table(tmp_path, capsys):
    from test_assign_host import CASES, DOC, N_REF, arrays
    case, z = CASES["joint_unlinked"], arrays()
    qr, qq = z["joint_unlinked_qr"], z["joint_unlinked_qq"]
    ref_edges = np.array(DOC["ref_edges"], dtype=np.int64)
    old = str(tmp_path / "old.csv")
    open(old, "w").write(DOC["old_csv"])
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=DOC["x_max"], optimal_y=DOC["y_max"])
    for sample in (None, 8):
        output = str(tmp_path / ("out_%s" % sample))
        os.makedirs(output)
        refnet = assign.ReferenceNetwork((ref_edges, N_REF), DOC["rNames"], old)
        qc_dict = {'run_qc': True, 'betweenness': True, 'max_merge': 0}
        if sample is not None:
            qc_dict['betweenness_sample'] = sample
        capsys.readouterr()
        res = assign.assign_query_clusters({'queryDatabase': lambda **kw: qq}, refnet, case["qNames"], qr, model, output,
                                           kmers=[13], qc_dict=qc_dict, return_network=True)
        text = capsys.readouterr().out
        assert res["isolateClustering"]["combined"] == case["expected"]["clustering"]
        edges, n = res["genomeNetwork"][:2]
        n_qry = len(case["qNames"])
        assert n == N_REF + n_qry
        k = sm.K_ALL if sample is None else sample
        want = sm.sampled_exact(np.asarray(edges), n, k, 0, whole=True)[0][N_REF:]
        start = text.index("query\tbetweenness\n")
        lines = text[start:].split("\n")[:n_qry + 1]
        got_names = [line.split("\t")[0] for line in lines[1:]]
        got_values = np.array([float(line.split("\t")[1]) for line in lines[1:]])
        # the table the reference prints over the device's own values: same text; its values: the model's
        table = assign.query_betweenness_table(case["qNames"], network.vertex_betweenness((edges, n), betweenness_sample=sample)[N_REF:])
        assert text[start:start + len(table)] == table
        assert sorted(got_names) == sorted(case["qNames"]) and np.all(np.diff(got_values) <= 0)
        by_name = dict(zip(case["qNames"], want))
        assert sm.bar_ratio(got_values, np.array([by_name[q] for q in got_names])) <= 1.0
