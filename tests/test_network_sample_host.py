"""CPU checks of tests/network_sample_model.py (no device) and of the Python plumbing of the sampled betweenness
(DESIGN.md 3.8): the sampling rule against hand values, the model against networkx 3.4.2 with the model's own source
list, the whole-graph model against networkx on disconnected graphs, every designed case of
tests/test_gpu_network_sample.py against the branch it names (read from the restated plan), and the mirrors' defaults,
errors and the assign table's text."""
import ctypes as C
import random
from fractions import Fraction
from operator import itemgetter

import numpy as np
import pytest

import network_model as nm
import network_sample_model as sm
from poppunk_amd import _lib, assign, engine, network, refine


# ---- the rule --------------------------------------------------------------------------------------------------------------
def test_hash_rule_by_hand():
    # splitmix64's published sequences: seeded with 0, and with 1234567 (its state after v + 1 steps is seed + (v + 1) G)
    seq0 = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    seq1 = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    assert [sm.sample_key(0, v) for v in range(3)] == [x >> 32 for x in seq0]
    assert [sm.sample_key(1234567, v) for v in range(5)] == [x >> 32 for x in seq1]
    assert sm.sample_key(0, 0) == 0xE220A839 and sm.sample_key(sm.GOLDEN, 0) == 0x6E789E6A
    assert sm.sample_key(2 ** 64 - 1, 0) == sm.fmix64(sm.GOLDEN - 1) >> 32          # the sum wraps mod 2^64


def test_sample_is_the_k_smallest_and_merges_to_a_subset():
    rng = np.random.default_rng(3)
    for seed in (0, 1, 99):
        a = sorted(rng.choice(5000, size=70, replace=False).tolist())
        b = sorted(set(rng.choice(5000, size=90, replace=False).tolist()) - set(a))
        for k in (1, 7, 69, 70, 71):
            sa = sm.sample_of(a, k, seed)
            assert sa == sorted(sa) and len(sa) == min(k, len(a)) and set(sa) <= set(a)
            if k < len(a):
                worst_in = max((sm.sample_key(seed, v), v) for v in sa)
                assert all((sm.sample_key(seed, v), v) > worst_in for v in set(a) - set(sa))
            merged = sm.sample_of(a + b, k, seed)
            if k < len(a) and k < len(b):
                assert set(merged) <= set(sa) | set(sm.sample_of(b, k, seed))
    # equal keys fall back on the id: the rule is a total order (a tie is forced by giving the same vertex twice a name)
    assert sm.sample_of([5, 3, 9], 3, 0) == [3, 5, 9] and sm.sample_of(range(10), 10, 4) == list(range(10))


# ---- the model against networkx ----------------------------------------------------------------------------------------------
class FixedSample(random.Random):
    """networkx draws its k sources with seed.sample(nodes, k): hand it the model's list"""

    def __new__(cls, sources):
        return super().__new__(cls, 0)

    def __init__(self, sources):
        super().__init__(0)
        self.sources = list(sources)

    def sample(self, population, k, **kw):
        assert k == len(self.sources) and set(self.sources) <= set(population)
        return list(self.sources)


def nx_graph(e, n):
    nx = pytest.importorskip("networkx")
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(np.asarray(e).tolist())
    return nx, G


@pytest.mark.parametrize("n,chords,k,seed", [(8, 2, 3, 0), (13, 5, 12, 1), (31, 10, 5, 2), (60, 25, 17, 3), (60, 0, 59, 4),
                                             (24, 30, 1, 5)])
def test_model_equals_networkx_with_the_same_sources(n, chords, k, seed):
    rng = np.random.default_rng(n + k)
    e, n_, _ = nm.assemble(n, [(nm.tree_with_chords(rng, n, chords), n)])
    nx, G = nx_graph(e, n_)
    assert nx.__version__ == "3.4.2" and nx.is_connected(G)
    want, summary, samples = sm.sampled_exact(e, n, k, seed)
    sources = samples[0]
    assert len(sources) == k
    got = nx.betweenness_centrality(G, k=k, normalized=True, seed=FixedSample(sources))
    assert sm.bar_ratio(np.array([got[v] for v in range(n)]), want) <= 1.0
    assert float(summary[0][0]) == want.max() and summary[0][1] == n
    # the float statement of the scale, against the exact one
    s = Fraction(12345, 7)
    assert sm.bar_ratio([sm.scaled_float(float(s), n, k)], [float(s * sm.scale_exact(n, k))]) <= 1.0
    # k >= n: every source, networkx without k
    full = nx.betweenness_centrality(G, normalized=True)
    assert sm.bar_ratio(np.array([full[v] for v in range(n)]), sm.sampled_exact(e, n, n, seed)[0]) <= 1.0
    assert np.array_equal(sm.sampled_exact(e, n, n, seed)[0], nm.brandes_exact(e, n)[0])


def test_whole_graph_model_equals_networkx_on_disconnected_graphs():
    e, n, ids = sm.case_whole()
    nx, G = nx_graph(e, n)
    assert sorted(len(c) for c in nx.connected_components(G)) == [1] * 5 + [2, 3, 3, 3, 4, 20]
    for norm in (True, False):
        got = nx.betweenness_centrality(G, normalized=norm)
        assert sm.bar_ratio(np.array([got[v] for v in range(n)]), sm.whole_exact(e, n, norm)) <= 1.0
    want = sm.whole_exact(e, n)
    for part in (6, 7):
        assert want[ids[part]].tolist() == [0.0, 2.0 / (39.0 * 38.0), 0.0]
    # the summary under the whole-graph flag is the per-component one
    assert sm.sampled_exact(e, n, 10, 0, whole=True)[1] == sm.sampled_exact(e, n, 10, 0)[1]
    # n <= 2: all 0; and a second mix with other sizes
    assert sm.whole_exact(np.array([[0, 1]]), 2).tolist() == [0.0, 0.0]
    e2, n2 = nm.many_components(6, 4, 9, seed=2, small=10)
    nx, G2 = nx_graph(e2, n2)
    got = nx.betweenness_centrality(G2)
    assert sm.bar_ratio(np.array([got[v] for v in range(n2)]), sm.whole_exact(e2, n2)) <= 1.0


# ---- every GPU case reaches the branch it names ----------------------------------------------------------------------------------
def test_rule_boundary_cases():
    for size in sm.RULE_SIZES:
        e, n = sm.case_rule_boundary(size)
        assert sm.sizes_adj_min(e, n)[0][0] == size and len(sm.sizes_adj_min(e, n)) == 1
        samples = sm.exact(sm.case_rule_boundary, sm.RULE_K, 0, False, size)[2]
        assert (len(samples) == 1 and len(next(iter(samples.values()))) == 100) if size == 101 else not samples


def test_multi_source_cases_reach_their_paths():
    e, n = nm.case_multi_source()
    sa = sm.sizes_adj_min(e, n)
    assert sa[0][0] == 120 and len(sa) == 301 and all(4 <= nc <= 9 for nc, _ in sa[1:])
    # k = 50, small_max = 8: the 120-vertex component walks its list in 256-thread items, 50 of them (the plan's target
    # is below one source of it), in LDS or on the slab; the 9-vertex components are exact items of 2 sources, the last
    # item short; the items are sized from 50 sources, not 120
    for lds_max, glob in ((0, 0), (100, 1)):
        p = sm.plan(sa, 8, lds_max, 50)
        assert p["K_glob"] == glob and p["K_big"] == 66 and p["sources"][0] == 50
        assert p["s"][0] == 1 and p["items"][0] == 50 != nm.plan(sa, 8, lds_max)["items"][0] == 120
        assert all((nc, s, it) == (9, 2, 5) for (nc, _), s, it in zip(sa[1:66], p["s"][1:66], p["items"][1:66]))
    # k = 5, small_max = 5: exactly the sampled components (n_c > 5) are 256-thread items, most of them of 1 < s = 2 < 5
    # listed sources with a short last item (2 + 2 + 1); lds_max = 3 puts every one on the slab
    for lds_max in (0, 3):
        p = sm.plan(sa, 5, lds_max, 5)
        assert p["K_big"] == 239 and p["K_glob"] == (239 if lds_max else 0)
        assert all(nc > 5 and src == 5 for (nc, _), src in zip(sa[:239], p["sources"][:239]))
        assert sum(1 for s, it in zip(p["s"][:239], p["items"][:239]) if (s, it) == (2, 3)) > 200
        assert all(nc <= 5 for nc, _ in sa[239:])
    # k = 5, default small_max (64): 120 > 64 goes to items, every smaller component to the one-wave path, those of more
    # than 5 vertices with a list, the rest exact
    p = sm.plan(sa, 64, 0, 5)
    assert p["K_big"] == 1 and p["K_glob"] == 0
    sampled = sum(1 for nc, _ in sa[1:] if nc > 5)
    assert 0 < sampled < 300
    assert len(sm.exact(nm.case_multi_source, 5, 0)[2]) == sampled + 1
    assert all(s == min(nc, 5) for s, (nc, _) in zip(p["s"][1:], sa[1:]))


def test_cap_cases():
    e, n = sm.case_cap()
    sa = sm.sizes_adj_min(e, n)
    assert [nc for nc, _ in sa] == [66, 65, 64]
    for k, n_sampled in ((64, 2), (65, 1)):
        p = sm.plan(sa, 64, 0, k)
        assert p["K_big"] == 2 and p["sources"] == [min(nc, k) for nc, _ in sa]
        assert len(sm.exact(sm.case_cap, k, 0)[2]) == n_sampled
    # k = 64: the 64-vertex component is one wave with every source (k <= n_c <= small_max holds with equality: no list)


def test_star_seeds_put_the_centre_in_and_out():
    e, n, centre = sm.case_star()
    assert np.bincount(e.reshape(-1), minlength=n)[centre] == 300 > 64           # a row longer than a wave
    seed_in, seed_out = sm.star_seeds()
    members = sm.components_min(e, n, 4)[0][0]
    assert centre in sm.sample_of(members, sm.STAR_K, seed_in)
    assert centre not in sm.sample_of(members, sm.STAR_K, seed_out)
    # centre out: n_c / (n_c - 1) at the centre, above 1; centre in: (k - 1) (n_c - 2) n_c / (k (n_c - 1)(n_c - 2))
    v_out = sm.exact(sm.case_star, sm.STAR_K, seed_out)[0]
    v_in = sm.exact(sm.case_star, sm.STAR_K, seed_in)[0]
    assert v_out[centre] == float(Fraction(301, 300)) and v_in[centre] == float(Fraction(6 * 301, 7 * 300))
    assert np.count_nonzero(v_out) == 1 and np.count_nonzero(v_in) == 1


def test_sweep_case_samples_and_merges():
    e, o, n, n_off = nm.case_reorder()
    sweeps = sm.exact_sweep(nm.case_reorder, 6, 0)
    assert sum(1 for t in range(n_off) if sweeps[t][2]) >= 8                    # sampled components at most levels
    assert len(sweeps[-1][1]) < max(len(s[1]) for s in sweeps)                  # components merge
    # the merged sample is a subset of the union of the earlier ones
    for t in range(1, n_off):
        before = set().union(*[set(s) for s in sweeps[t - 1][2].values()]) if sweeps[t - 1][2] else set()
        small_before = {v for c in sm.components_min(e[o <= t - 1], n, 1)[0] if len(c) <= 6 for v in c}
        for s in sweeps[t][2].values():
            assert set(s) <= before | small_before


# ---- the plumbing ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_argument_errors_need_no_device():
    for name in ("ppk_network_summary_sampled_dev", "ppk_network_summary_sampled"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    lib = _lib.lib()
    with pytest.raises(RuntimeError, match="ppk_network_summary_sampled: bt_sources must be >= 1"):
        _lib.check(lib.ppk_network_summary_sampled(None, None, None, 0, 4, 1, 0, -1, None, None, None, None, 0, 0, 0), "x")
    with pytest.raises(RuntimeError, match="ppk_network_summary_sampled: unknown flag bits"):
        _lib.check(lib.ppk_network_summary_sampled(None, None, None, 0, 4, 1, 0, -1, None, None, None, None, 5, 0, 2), "x")
    with pytest.raises(RuntimeError, match="ppk_network_summary_sampled: bt_sources must be >= 1"):
        _lib.check(lib.ppk_network_summary_sampled_dev(None, None, 1, None, 0, 4, 1, -1, None, None, None, None, 0, 0, 0,
                                                       None), "x")
    with pytest.raises(RuntimeError, match="ppk_network_summary_sampled: NULL array"):
        _lib.check(lib.ppk_network_summary_sampled(None, None, None, 0, 4, 1, 0, -1, None, None, None, None, 5, 0, 1), "x")
    e = np.array([[0, 1], [1, 2]], dtype=np.int64)
    with pytest.raises(ValueError):
        refine.network_summary_sampled(e[:, 0], e[:, 1], None, 4, sources=0)
    with pytest.raises(ValueError):
        network.networkSummary((e, 4), sampled_betweenness=True, betweenness_sample=0)
    with pytest.raises(ValueError):
        network.vertex_betweenness((e, 4), betweenness_sample=0)
    with pytest.raises(ValueError):
        engine.network_summary_sampled_dev(None, None, None, 4, 1, sources=0)


def test_defaults_call_the_old_functions_with_the_old_arguments(monkeypatch):
    e = np.array([[0, 1], [1, 2], [2, 3], [3, 4]], dtype=np.int64)
    calls = []

    def old(*a, **kw):
        calls.append(("old", a, kw))
        return np.array([[4, 1, 0, 3]]), np.array([[0.5, 0.5]]), None, None

    def new(*a, **kw):
        calls.append(("new", a, kw))
        return np.array([[4, 1, 0, 3]]), np.array([[0.25, 0.25]]), None, None
    monkeypatch.setattr(refine, "network_summary", old)
    monkeypatch.setattr(refine, "network_summary_sampled", new)
    for kw in ({}, {"betweenness_sample": 2}, {"betweenness_sample": 2, "seed": 9, "use_gpu": True}):
        calls.clear()
        metrics, _ = network.networkSummary((e, 5), **kw)
        (which, a, k), = calls
        assert which == "old" and k == {} and len(a) == 5 and a[2] is None and a[3:] == (5, 1) and metrics[3] == 0.5
        assert np.array_equal(a[0], e[:, 0]) and np.array_equal(a[1], e[:, 1])
    calls.clear()
    metrics, _ = network.networkSummary((e, 5), sampled_betweenness=True, betweenness_sample=2, seed=9)
    (which, a, k), = calls
    assert which == "new" and k == {"sources": 2, "seed": 9} and a[2:] == (None, 5, 1) and metrics[3] == 0.25
    calls.clear()
    network.print_network_summary((e, 5))
    network.print_network_summary((e, 5), sampled_betweenness=True, betweenness_sample=3)
    assert [c[0] for c in calls] == ["old", "new"] and calls[1][2] == {"sources": 3, "seed": 0}
    calls.clear()
    network.networkSummary((e, 5), calc_betweenness=False, sampled_betweenness=True) if False else None
    # the sweeps: the default reaches network_summary_dev with today's arguments
    seen = []

    class Dist:
        shape = (10, 2)
    monkeypatch.setattr(engine, "network_summary_dev", lambda *a, **kw: seen.append(("old", a, kw)) or (FakeT(), FakeT(), 0, 0))
    monkeypatch.setattr(engine, "network_summary_sampled_dev",
                        lambda *a, **kw: seen.append(("new", a, kw)) or (FakeT(), FakeT(), 0, 0))
    monkeypatch.setattr(refine, "grow_scores", lambda *a, **kw: [0.0])
    engine._sweep_scores(Dist(), ("i", "j", "o"), 3, 1)
    engine._sweep_scores(Dist(), ("i", "j", "o"), 3, 2, 7, 11)
    assert seen[0] == ("old", ("i", "j", "o", 5, 3), {})
    assert seen[1] == ("new", ("i", "j", "o", 5, 3), {"sources": 7, "seed": 11})


class FakeT:
    def cpu(self):
        return self

    def numpy(self):
        return np.zeros((3, 4))


def test_subsample_still_raises_before_the_device(monkeypatch):
    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    e = np.array([[0, 1], [1, 2]], dtype=np.int64)
    with pytest.raises(NotImplementedError):
        network.networkSummary((e, 4), subsample=2, sampled_betweenness=True)
    with pytest.raises(NotImplementedError):
        network.print_network_summary((e, 4), sample_size=2, sampled_betweenness=True)
    with pytest.raises(NotImplementedError):
        refine.refineFit(None, ["a"] * 4, (0.1, 0.1), (0.5, 0.5), np.ones(2), 0.1, 0.05, score_idx=1, sample_size=2,
                         sampled_betweenness=True)


class StandInScorer:
    """refineFit's scorer with the sweep's minimum at the last offset: no local search"""
    n_rows = 10

    def __init__(self, settable=True):
        self.set = []
        if settable:
            self.set_betweenness_sample = lambda k, seed=0: self.set.append((k, seed))

    def sweep_1d(self, s_range, slope, mean0, mean1, score_idx):
        return 5, [-0.01 * t for t in range(len(s_range))]


def test_refine_fit_records_the_mode(capsys):
    args = (["s%d" % k for k in range(5)], (0.1, 0.1), (0.5, 0.5), np.ones(2), 0.1, 0.05)
    scorer = StandInScorer()
    refine.refineFit(scorer, *args, score_idx=1)
    assert scorer.set == [(None, 0)]
    assert (refine.last_fit["betweenness"], refine.last_fit["betweenness_sample"], refine.last_fit["seed"]) == \
        ("exact", None, None)
    refine.refineFit(scorer, *args, score_idx=2, sampled_betweenness=True, betweenness_sample=25, seed=4)
    assert scorer.set[-1] == (25, 4)
    assert (refine.last_fit["betweenness"], refine.last_fit["betweenness_sample"], refine.last_fit["seed"]) == \
        ("sampled", 25, 4)
    refine.refineFit(scorer, *args, score_idx=0, sampled_betweenness=True)       # score_idx 0 computes no betweenness
    assert scorer.set[-1] == (None, 0) and refine.last_fit["betweenness"] == "exact"
    refine.refineFit(StandInScorer(settable=False), *args, score_idx=1)           # a four-method stand-in still works
    with pytest.raises(TypeError):
        refine.refineFit(StandInScorer(settable=False), *args, score_idx=1, sampled_betweenness=True)
    with pytest.raises(ValueError):
        refine.refineFit(scorer, *args, score_idx=1, sampled_betweenness=True, betweenness_sample=0)


def test_assign_table_text_and_order():
    e, n, _ = sm.case_whole()
    values = sm.whole_exact(e, n)
    qNames = ["q%02d" % k for k in range(12)]
    q_values = values[n - 12:]
    assert len(set(q_values.tolist())) < 12                                   # ties (several zeros)
    # PopPUNK/assign.py:646-651, restated over the same values
    query_betweenness = {query: b for query, b in zip(qNames, q_values)}
    want = "query\tbetweenness\n"
    for query, q_betweenness in sorted(query_betweenness.items(), key=itemgetter(1), reverse=True):
        want += f"{query}\t{q_betweenness}\n"
    assert assign.query_betweenness_table(qNames, q_values) == want == sm.betweenness_table(qNames, q_values)
    rows = want.split("\n")[1:-1]
    zeros = [r.split("\t")[0] for r in rows if float(r.split("\t")[1]) == 0.0]
    assert zeros == sorted(zeros) and len(zeros) > 1                          # equal values keep the queries' order
    assert assign.query_betweenness_table(["a", "b"], [0.0, 0.5]) == "query\tbetweenness\nb\t0.5\na\t0.0\n"
