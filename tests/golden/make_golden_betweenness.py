#!/usr/bin/env python3
"""Generates tests/golden/network_betweenness.npz: networkSummary with betweenness as the reference computes it.

Run in the BUILD container only (needs the reference checkout, networkx and pandas); the fixture it writes is data
and is committed, the reference is not.  It reuses make_golden_network.py's helpers (ast extraction, the networkx
stand-in for graph-tool, the tqdm stub) and runs, unmodified:
  PopPUNK/network.py  networkSummary, vertex_betweenness, print_network_summary, construct_network_from_df,
                      construct_network_from_edge_list
  PopPUNK/refine.py   growNetwork
The stand-in is extended with what the betweenness branch (network.py:1286-1307) calls:
  label_components(g)      -> (labels with .a, sizes), labels numbered as the sizes list is ordered
  GraphView(g, vfilt=...)  -> the subgraph on the vertices where vfilt is True
  betweenness(g, norm=True) -> networkx betweenness_centrality(normalized=norm): sum over all sources of the pair
                              dependencies / ((n - 1)(n - 2)).  That graph-tool's betweenness(norm=True) returns the
                              same values is UNVERIFIED (graph-tool is not in this image).

Arrays (prefix `<case>_`):
  sweep1d, sweep2d   the triples of network_sweep.npz (the GPU test chains them from that file's distance matrices);
                     present (the offset indices growNetwork scores), metrics float64 [len(present), 5] (networkSummary
                     with betweenness at each), scores1 / scores2 (growNetwork's list for score_idx 1 / 2), bt float64
                     [n_off, 2] (metrics 3 and 4 of the graph at every offset, an offset without edges repeating the
                     one before it; zeros before the first)
  mix, tiny          single graphs: edges int64 [m, 2], n, metrics [5], scores [3], values float64 [n] (every
                     vertex's normalised betweenness within its component, 0 in components of <= 3 vertices), stats
                     (edges, components, triangles, connected triples, from networkx), scored
                     (components of > 3 vertices) and text (print_network_summary's stderr).  mix has two dense
                     clusters, a long path, a star, a 4-vertex path, a clique and many components of 1-6 vertices;
                     tiny only single edges and isolated vertices: no connected triple (transitivity NaN).
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_network as mgn  # noqa: E402


class _Prop:
    def __init__(self, a):
        self.a = np.asarray(a)


class _FakeGtBt(mgn._FakeGt):
    """make_golden_network's stand-in plus the betweenness branch's calls."""

    @staticmethod
    def label_components(g):
        import networkx as nx
        comps = [sorted(c) for c in nx.connected_components(g.g)]
        lab = np.zeros(g.g.number_of_nodes(), dtype=np.int64)
        nodes = list(g.g.nodes())
        pos = {v: k for k, v in enumerate(nodes)}
        for k, c in enumerate(comps):
            for v in c:
                lab[pos[v]] = k
        return _Prop(lab), [len(c) for c in comps]

    @staticmethod
    def GraphView(g, vfilt):
        nodes = list(g.g.nodes())
        keep = [nodes[k] for k in np.flatnonzero(np.asarray(vfilt))]
        view = mgn._FakeGt.Graph.__new__(mgn._FakeGt.Graph)
        view.g = g.g.subgraph(keep).copy()
        return view

    @staticmethod
    def betweenness(g, norm=True):
        import networkx as nx
        bc = nx.betweenness_centrality(g.g, normalized=norm)
        return _Prop([bc[v] for v in g.g.nodes()]), None


def namespace(record):
    import pandas as pd
    ns = {"np": np, "pd": pd, "gt": _FakeGtBt, "tqdm": mgn._Tqdm, "os": os, "sys": sys,
          "betweenness_sample_default": 100}
    mgn.extract_functions(os.path.join(mgn.REF, "PopPUNK", "network.py"),
                          ["construct_network_from_df", "construct_network_from_edge_list", "networkSummary",
                           "vertex_betweenness", "print_network_summary"], ns)
    mgn.extract_functions(os.path.join(mgn.REF, "PopPUNK", "refine.py"), ["growNetwork"], ns)
    summary = ns["networkSummary"]

    def recording_summary(G, *a, **kw):
        out = summary(G, *a, **kw)
        record.append(out[0])
        return out
    ns["networkSummary"] = recording_summary
    return ns


def graph(ns, edges, n):
    G = _FakeGtBt.Graph(directed=False)
    G.add_vertex(n)
    G.add_edge_list([tuple(e) for e in edges.tolist()])
    return G


def sweep_case(z, case):
    i, j, idx, n = z[case + "_i"], z[case + "_j"], z[case + "_idx"], int(z[case + "_n"])
    n_off = int(z[case + "_n_off"])
    names = ["s%d" % k for k in range(n)]
    out = {}
    for score_idx in (1, 2):
        record = []
        ns = namespace(record)
        out["scores%d" % score_idx] = np.array(
            ns["growNetwork"](names, i.tolist(), j.tolist(), idx.tolist(), list(range(n_off)), score_idx=score_idx),
            dtype=np.float64)
        out["metrics"] = np.array(record, dtype=np.float64)
    present = np.unique(idx)
    assert out["metrics"].shape[0] == present.size
    bt = np.zeros((n_off, 2))
    row = np.zeros(2)
    for t in range(n_off):
        hit = np.flatnonzero(present == t)
        if hit.size:
            row = out["metrics"][hit[0], 3:5]
        bt[t] = row
    out.update(present=present.astype(np.int64), bt=bt)
    return out


def single_case(edges, n):
    import networkx as nx
    record = []
    ns = namespace(record)
    G = graph(ns, edges, n)
    metrics, scores = ns["networkSummary"](G)
    text = io.StringIO()
    with contextlib.redirect_stderr(text):
        ns["print_network_summary"](G)
    values = np.zeros(n)
    scored = 0
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges.tolist())
    for c in nx.connected_components(g):
        if len(c) > 3:
            scored += 1
            for v, b in nx.betweenness_centrality(g.subgraph(c), normalized=True).items():
                values[v] = b
    stats = mgn.stats_per_offset(edges[:, 0], edges[:, 1], np.zeros(edges.shape[0], dtype=np.int64), n, 1)[0]
    return {"edges": edges.astype(np.int64), "n": np.int64(n), "stats": stats,
            "metrics": np.array(metrics, dtype=np.float64),
            "scores": np.array(scores, dtype=np.float64), "values": values, "scored": np.int64(scored),
            "text": np.array(text.getvalue())}


def mixed_graph(seed):
    rng = np.random.default_rng(seed)
    edges = []
    at = [0]

    def take(k):
        v = list(range(at[0], at[0] + k))
        at[0] += k
        return v

    for size, p in ((40, 0.45), (25, 0.7)):                    # dense clusters
        v = take(size)
        for a in range(size):
            for b in range(a + 1, size):
                if rng.random() < p or b == a + 1:
                    edges.append((v[a], v[b]))
    v = take(150)                                             # a long path
    edges += [(v[k], v[k + 1]) for k in range(149)]
    v = take(13)                                              # a star
    edges += [(v[0], v[k]) for k in range(1, 13)]
    v = take(4)                                               # a 4-vertex path
    edges += [(v[0], v[1]), (v[1], v[2]), (v[2], v[3])]
    v = take(9)                                               # a clique
    edges += [(v[a], v[b]) for a in range(9) for b in range(a + 1, 9)]
    for _ in range(120):                                      # components of 1-6 vertices
        size = int(rng.integers(1, 7))
        v = take(size)
        for k in range(1, size):
            edges.append((v[int(rng.integers(0, k))], v[k]))
        if size > 3 and rng.random() < 0.5:
            edges.append((v[0], v[size - 1]))
    edges = np.array(sorted(set((min(a, b), max(a, b)) for a, b in edges)), dtype=np.int64)
    perm = rng.permutation(at[0])                             # ids scattered over the vertex range
    edges = perm[edges]
    return edges[rng.permutation(edges.shape[0])], at[0]


def main():
    z = np.load(os.path.join(HERE, "network_sweep.npz"))
    out = {}
    for case in ("sweep1d", "sweep2d"):
        for k, v in sweep_case(z, case).items():
            out["%s_%s" % (case, k)] = v
    edges, n = mixed_graph(7)
    for k, v in single_case(edges, n).items():
        out["mix_" + k] = v
    tiny = np.array([(0, 1), (2, 3), (6, 7), (9, 10), (12, 11)], dtype=np.int64)
    for k, v in single_case(tiny, 14).items():
        out["tiny_" + k] = v
    path = os.path.join(HERE, "network_betweenness.npz")
    np.savez_compressed(path, **out)
    for case in ("sweep1d", "sweep2d"):
        print(case, "present", out[case + "_present"].size, "scores", out[case + "_scores1"].size,
              "bt max", out[case + "_bt"].max())
    for case in ("mix", "tiny"):
        print(case, "n", int(out[case + "_n"]), "edges", out[case + "_edges"].shape[0], "metrics",
              out[case + "_metrics"].tolist())
        print(str(out[case + "_text"]))


if __name__ == "__main__":
    main()
