"""GPU tests of networkSummary's betweenness on the device (ppk_network_summary_dev): per-vertex values
and per-offset means against a pure-Python Brandes under every forced path, the counts bit for bit against
ppk_network_sweep_dev, bit-identical repeats whatever the edge order, the reference-derived golden
(tests/golden/network_betweenness.npz) through refine_sweep_scores_dev(score_idx=1|2) and network.networkSummary, the
exact small cases, and the argument errors."""
import os
from collections import deque

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, network, refine  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "network_betweenness.npz")
SWEEP = os.path.join(HERE, "golden", "network_sweep.npz")
DEV = "cuda:0"

# (bt_lds_max, bt_small_max): default; everything in the global-state path; small path off; LDS path for all but tiny
PATHS = [(0, 64), (3, 0), (0, 0), (5, 64), (0, 256)]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def brandes(edges, n):
    """normalised betweenness of every vertex within its component (0 in components of <= 3 vertices), and per
    component of > 3 vertices its (max, size)"""
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        adj[a].append(b)
        adj[b].append(a)
    comp = [-1] * n
    comps = []
    for v in range(n):
        if comp[v] >= 0:
            continue
        comp[v] = len(comps)
        members, todo = [v], [v]
        while todo:
            u = todo.pop()
            for w in adj[u]:
                if comp[w] < 0:
                    comp[w] = comp[v]
                    members.append(w)
                    todo.append(w)
        comps.append(members)
    bc = [0.0] * n
    summary = []
    for members in comps:
        nc = len(members)
        if nc <= 3:
            continue
        acc = {v: 0.0 for v in members}
        for s in members:
            sigma = {s: 1.0}
            dist = {s: 0}
            order = []
            pred = {v: [] for v in members}
            q = deque([s])
            while q:
                u = q.popleft()
                order.append(u)
                for w in adj[u]:
                    if w not in dist:
                        dist[w] = dist[u] + 1
                        q.append(w)
                    if dist[w] == dist[u] + 1:
                        sigma[w] = sigma.get(w, 0.0) + sigma[u]
                        pred[w].append(u)
            delta = {v: 0.0 for v in members}
            for w in reversed(order):
                for u in pred[w]:
                    delta[u] += sigma[u] / sigma[w] * (1 + delta[w])
                if w != s:
                    acc[w] += delta[w]
        scale = 1.0 / ((nc - 1) * (nc - 2))
        for v in members:
            bc[v] = acc[v] * scale
        summary.append((max(bc[v] for v in members), nc))
    return np.array(bc), summary


def means(summary):
    if not summary:
        return 0.0, 0.0
    b = np.array([x for x, _ in summary])
    w = np.array([s for _, s in summary], dtype=np.float64)
    return float(b.mean()), float((b * w).sum() / w.sum())


def clustered_graph(rng, n_clusters=6, chain=60, tiny=40):
    """dense clusters, a chain, a few bridges, and tiny components; ids shuffled; each unordered pair once"""
    edges, at = [], 0
    for _ in range(n_clusters):
        size = int(rng.integers(5, 60))
        p = rng.uniform(0.2, 0.9)
        for a in range(size):
            for b in range(a + 1, size):
                if rng.random() < p or b == a + 1:
                    edges.append((at + a, at + b))
        at += size
    edges += [(at + k, at + k + 1) for k in range(chain - 1)]
    edges.append((at, at - 1))                      # the chain hangs off the last cluster
    at += chain
    for _ in range(tiny):
        size = int(rng.integers(1, 7))
        for k in range(1, size):
            edges.append((at + int(rng.integers(0, k)), at + k))
        at += size
    e = np.array(sorted(set((min(a, b), max(a, b)) for a, b in edges)), dtype=np.int64)
    perm = rng.permutation(at)
    e = perm[e]
    swap = rng.random(e.shape[0]) < 0.5
    e[swap] = e[swap][:, ::-1]
    return e[rng.permutation(e.shape[0])], at


def check_values(got, want):
    got = np.asarray(got)
    err = np.abs(got - want)
    assert np.all(err <= np.maximum(1e-12 * np.abs(want), 1e-15)), float(err.max())


@pytest.mark.parametrize("lds_max,small_max", PATHS)
def test_values_equal_python_brandes_on_every_path(lds_max, small_max, ppk_option):
    ppk_option("bt_lds_max", lds_max)
    ppk_option("bt_small_max", small_max)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        e, n = clustered_graph(rng)
        want, summary = brandes(e, n)
        stats, bt, scored, values = engine.network_summary_graph_dev(dev(e), n, values=True)
        check_values(values.cpu().numpy(), want)
        assert int(scored) == len(summary)
        np.testing.assert_allclose(bt.cpu().numpy(), means(summary), rtol=1e-12, atol=1e-15)
        ref_stats, _ = engine.network_stats_dev(dev(e), n)
        assert torch.equal(stats, ref_stats)


def growing_sweep(rng, n_off=40):
    e, n = clustered_graph(rng, n_clusters=5, chain=40, tiny=30)
    used = np.sort(rng.choice(n_off, size=(2 * n_off) // 3, replace=False))
    o = rng.choice(used, size=e.shape[0]).astype(np.int64)
    return e, o, n, n_off


def test_sweep_means_equal_brute_force_and_stats_equal_the_sweep(ppk_option):
    rng = np.random.default_rng(3)
    e, o, n, n_off = growing_sweep(rng)
    stats, bt, scored, values = engine.network_summary_dev(dev(e[:, 0]), dev(e[:, 1]), dev(o), n, n_off, values_at=20)
    ref, _ = engine.network_sweep_dev(dev(e[:, 0]), dev(e[:, 1]), dev(o), n, n_off)
    assert torch.equal(stats, ref)
    bt, scored = bt.cpu().numpy(), scored.cpu().numpy()
    for t in range(n_off):
        want_v, summary = brandes(e[o <= t], n)
        np.testing.assert_allclose(bt[t], means(summary), rtol=1e-12, atol=1e-15, err_msg=str(t))
        assert scored[t] == len(summary), t
        if t == 20:
            check_values(values.cpu().numpy(), want_v)
    # host arrays: the same numbers
    hs, hb, hsc, hv = refine.network_summary(e[:, 0], e[:, 1], o, n, n_off, values_at=20)
    assert np.array_equal(hs, stats.cpu().numpy())
    assert np.array_equal(hb, bt) and np.array_equal(hsc, scored)
    assert np.array_equal(hv, values.cpu().numpy())
    # every forced path: within rounding of the default
    for lds_max, small_max in PATHS[1:]:
        ppk_option("bt_lds_max", lds_max)
        ppk_option("bt_small_max", small_max)
        _, b2, s2, _ = engine.network_summary_dev(dev(e[:, 0]), dev(e[:, 1]), dev(o), n, n_off)
        np.testing.assert_allclose(b2.cpu().numpy(), bt, rtol=1e-12, atol=1e-15)
        assert np.array_equal(s2.cpu().numpy(), scored)


def test_repeats_and_edge_order_give_the_same_bits():
    rng = np.random.default_rng(4)
    e, o, n, n_off = growing_sweep(rng)
    first = engine.network_summary_dev(dev(e[:, 0]), dev(e[:, 1]), dev(o), n, n_off, values_at=n_off - 1)
    for _ in range(2):
        again = engine.network_summary_dev(dev(e[:, 0]), dev(e[:, 1]), dev(o), n, n_off, values_at=n_off - 1)
        for a, b in zip(first, again):
            assert torch.equal(a, b)
    perm = rng.permutation(e.shape[0])
    pe, po = e[perm][:, ::-1], o[perm]                # permuted, and (i, j) swapped
    other = engine.network_summary_dev(dev(pe[:, 0]), dev(pe[:, 1]), dev(po), n, n_off, values_at=n_off - 1)
    for a, b in zip(first, other):
        assert torch.equal(a, b)


def assert_scores(got, want):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=1e-15)


def test_golden_sweeps_through_refine_sweep_scores():
    g, z = np.load(GOLDEN), np.load(SWEEP)
    x0, y0, x1, y1 = z["sweep1d_line"]
    for score_idx in (1, 2):
        stats, scores = engine.refine_sweep_scores_dev(dev(z["sweep1d_dist"]), z["sweep1d_offsets"], 2, x0, y0, x1, y1,
                                                       score_idx=score_idx)
        assert np.array_equal(stats.cpu().numpy(), z["sweep1d_stats"])
        assert_scores(scores, g["sweep1d_scores%d" % score_idx])
        stats, scores = engine.refine_sweep_scores_2d_dev(dev(z["sweep2d_dist"]), z["sweep2d_xmax"],
                                                          float(z["sweep2d_ymax"]), score_idx=score_idx)
        assert np.array_equal(stats.cpu().numpy(), z["sweep2d_stats"])
        assert_scores(scores, g["sweep2d_scores%d" % score_idx])
    # the default leaves today's scores
    _, scores = engine.refine_sweep_scores_dev(dev(z["sweep1d_dist"]), z["sweep1d_offsets"], 2, x0, y0, x1, y1)
    assert_scores(scores, z["sweep1d_scores"])
    for case in ("sweep1d", "sweep2d"):
        n, n_off = int(z[case + "_n"]), int(z[case + "_n_off"])
        stats, bt, _, _ = refine.network_summary(z[case + "_i"], z[case + "_j"], z[case + "_idx"], n, n_off)
        np.testing.assert_allclose(bt, g[case + "_bt"], rtol=1e-12, atol=1e-15)
        for t, want in zip(g[case + "_present"], g[case + "_metrics"]):
            metrics, _ = refine.summary_from_stats(stats[t], n, bt[t])
            assert metrics[0] == want[0] and metrics[1] == want[1]
            np.testing.assert_allclose(metrics[3:], want[3:], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("case", ["mix", "tiny"])
def test_golden_network_summary(case):
    g = np.load(GOLDEN)
    e, n = g[case + "_edges"], int(g[case + "_n"])
    for edges in (e, dev(e)):
        metrics, scores = network.networkSummary((edges, n))
        want = g[case + "_metrics"]
        assert metrics[0] == want[0] and metrics[1] == want[1]
        assert (np.isnan(metrics[2]) and np.isnan(want[2])) or metrics[2] == want[2]
        np.testing.assert_allclose(metrics[3:], want[3:], rtol=1e-12, atol=1e-15)
        assert_scores(scores, g[case + "_scores"])
    _, _, scored, values = engine.network_summary_graph_dev(dev(e), n, values=True)
    check_values(values.cpu().numpy(), g[case + "_values"])
    assert int(scored) == int(g[case + "_scored"])
    # without betweenness: metrics 3 and 4 are 0, as in the reference
    metrics, _ = network.networkSummary((e, n), calc_betweenness=False)
    assert metrics[3] == 0 and metrics[4] == 0


def test_print_network_summary_writes_the_reference_text(capsys):
    g = np.load(GOLDEN)
    for case in ("mix", "tiny"):
        network.print_network_summary((dev(g[case + "_edges"]), int(g[case + "_n"])))
        assert capsys.readouterr().err == str(g[case + "_text"])


def test_exact_cases():
    star = np.array([(0, k) for k in range(1, 9)], dtype=np.int64)
    _, bt, scored, v = engine.network_summary_graph_dev(dev(star), 9, values=True)
    assert v[0].item() == 1.0 and torch.all(v[1:] == 0).item()
    assert bt.tolist() == [1.0, 1.0] and int(scored) == 1
    path = np.array([(0, 1), (1, 2), (2, 3)], dtype=np.int64)
    _, bt, _, v = engine.network_summary_graph_dev(dev(path), 4, values=True)
    np.testing.assert_allclose(v.cpu().numpy(), [0, 2 / 3, 2 / 3, 0], rtol=1e-15, atol=0)
    clique = np.array([(a, b) for a in range(7) for b in range(a + 1, 7)], dtype=np.int64)
    _, bt, scored, v = engine.network_summary_graph_dev(dev(clique), 7, values=True)
    assert torch.all(v == 0).item() and bt.tolist() == [0.0, 0.0] and int(scored) == 1
    small = np.array([(0, 1), (1, 2), (4, 5), (7, 8), (8, 9)], dtype=np.int64)
    stats, bt, scored, v = engine.network_summary_graph_dev(dev(small), 11, values=True)
    assert torch.all(v == 0).item() and bt.tolist() == [0.0, 0.0] and int(scored) == 0
    assert stats.tolist() == [5, 6, 0, 2]
    e = torch.zeros((0, 2), dtype=torch.int64, device=DEV)
    stats, bt, scored, v = engine.network_summary_graph_dev(e, 6, values=True)
    assert stats.tolist() == [0, 6, 0, 0] and bt.tolist() == [0.0, 0.0] and int(scored) == 0
    assert torch.all(v == 0).item()
    z = torch.zeros(0, dtype=torch.int64, device=DEV)
    stats, bt, scored, _ = engine.network_summary_dev(z, z, z, 9, 5)
    assert bt.tolist() == [[0.0, 0.0]] * 5 and scored.tolist() == [0] * 5
    # n_off = 1 without offsets, on separate arrays; and an [m, 2] strided view of a wider tensor's columns
    _, bt1, _, _ = engine.network_summary_dev(dev(star[:, 0]), dev(star[:, 1]), None, 9, 1)
    assert bt1.tolist() == [[1.0, 1.0]]
    wide = dev(np.concatenate([star, star], axis=1))[:, :2]
    with pytest.raises(TypeError):
        engine.network_summary_graph_dev(wide, 9)
    view = dev(star)
    _, bt2, _, _ = engine.network_summary_dev(view[:, 0], view[:, 1], None, 9, 1)
    assert torch.equal(bt1, bt2)
    # an offset without edges repeats the row before it; values at it are those of the graph before it
    o = dev(np.array([0, 0, 0, 2, 2, 2, 2, 2], dtype=np.int64))
    _, bt, scored, v = engine.network_summary_dev(view[:, 0], view[:, 1], o, 9, 4, values_at=1)
    assert bt.tolist() == [[1.0, 1.0]] * 4 and scored.tolist() == [1, 1, 1, 1]
    assert v[0].item() == 1.0


def test_errors_name_an_edge_and_the_next_call_succeeds():
    lib = _lib.lib()
    i = dev(np.array([0, 1, 2, 3], dtype=np.int64))
    j = dev(np.array([1, 2, 3, 0], dtype=np.int64))
    o = dev(np.array([0, 1, 1, 2], dtype=np.int64))
    st = torch.zeros((8, 4), dtype=torch.int64, device=DEV)
    bt = torch.zeros((8, 2), dtype=torch.float64, device=DEV)
    sc = torch.zeros(8, dtype=torch.int64, device=DEV)
    val = torch.zeros(8, dtype=torch.float64, device=DEV)

    def call(i_t, j_t, o_t, n, n_off, values_at=-1):
        return lib.ppk_network_summary_dev(i_t.data_ptr(), j_t.data_ptr(), 1, o_t.data_ptr() if o_t is not None else None,
                                           i_t.shape[0], n, n_off, values_at, st.data_ptr(), bt.data_ptr(),
                                           sc.data_ptr(), val.data_ptr(), None)

    cases = [((i, dev(np.array([1, 2, 9, 0], dtype=np.int64)), o, 5, 3), b"edge 2"),
             ((i, dev(np.array([1, 2, 2, 0], dtype=np.int64)), o, 5, 3), b"self-loop"),
             ((i, j, dev(np.array([0, 1, 3, 2], dtype=np.int64)), 5, 3), b"offset"),
             ((i, j, o, 5, 0), b"n_off"), ((i, j, o, 5, 1024), b"n_off"), ((i, j, None, 5, 3), b"n_off"),
             ((i, j, o, 5, 3, 3), b"values_at")]
    for args, msg in cases:
        assert call(*args) == _lib.ERR_ARG, msg
        assert msg in lib.ppk_last_error(), (msg, lib.ppk_last_error())
        assert b"ppk_network_summary" in lib.ppk_last_error(), lib.ppk_last_error()
        assert call(i, j, o, 5, 3, 2) == _lib.OK
        torch.cuda.synchronize()
        assert st[:3].tolist() == [[1, 4, 0, 0], [3, 2, 0, 2], [4, 2, 0, 4]]
        # G_1: the path 0-1-2-3 (inner vertices 2/3); G_2: the 4-cycle 0-1-2-3 and the isolated 4, every cycle vertex
        # 1 / ((4 - 1)(4 - 2)) = 1/6
        np.testing.assert_allclose(bt[:3].cpu().numpy(), [[0, 0], [2 / 3, 2 / 3], [1 / 6, 1 / 6]], rtol=1e-15, atol=0)
        np.testing.assert_allclose(val[:5].cpu().numpy(), [1 / 6] * 4 + [0], rtol=1e-15, atol=0)
    with pytest.raises(RuntimeError, match="ppk_network_summary_dev"):
        engine.network_summary_dev(i, dev(np.array([1, 2, 9, 0], dtype=np.int64)), o, 5, 3)
