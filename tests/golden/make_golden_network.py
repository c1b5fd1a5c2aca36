#!/usr/bin/env python3
"""Generates tests/golden/network_sweep.npz: refine.growNetwork's score lists as the reference computes them.

Run in the BUILD container only (needs the reference checkout, networkx and pandas); the fixture it writes is data
(edge triples, n, per-offset counts, metrics and score lists) and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast`, as make_golden_bgmm.py does, and run unmodified):
  PopPUNK/refine.py   growNetwork
  PopPUNK/network.py  construct_network_from_df, construct_network_from_edge_list, networkSummary
under the real pandas / numpy of this image and a small stand-in for graph-tool built on networkx (graph-tool is not
in this image): Graph, add_vertex, add_edge_list, vertices, edges, label_components, and global_clustering = 3T / W
with NaN when W = 0 -- that last value is the stand-in's, unverified against graph-tool.  tqdm is a no-op stub.

Cases (prefix `<case>_` on every array; `cases` lists them):
  sweep1d   oracle.threshold_iterate_1d triples (40 offsets) on a synthetic clustered distance matrix, n = 300
  sweep2d   oracle.threshold_iterate_2d triples (20 x values, one y) on another, n = 200
  holes     the 1-D triples of n = 120 with every edge of offsets 3-5, 9 and 17 removed: offset indices that never
            occur take the score of the next one that does (refine.py:463)
  late      the same triples without offsets 0-6: the list starts with idx + 1 copies of the first score
Per case: i, j, idx (the triples), n, n_off, stats int64 [n_off, 4] (edges, components, triangles, connected triples
of the graph of every edge with index <= t, from networkx), present (the offset indices growNetwork scores),
metrics float64 [len(present), 5] (networkSummary's metrics at each of them) and scores (growNetwork's list).
sweep1d and sweep2d also keep their distance matrix and sweep arguments (dist, offsets + line x0 y0 x1 y1; dist,
xmax, ymax), so the device sweep can be chained into the scores.
"""
import ast
import os
import sys

import numpy as np

REF = os.environ.get("POPPUNK_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def extract_functions(path, names, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    missing = [n for n in names if n not in namespace]
    if missing:
        raise RuntimeError("not found in %s: %s" % (path, missing))
    return namespace


class _FakeGt:
    """The part of graph_tool the extracted functions call, on networkx."""

    class Graph:
        def __init__(self, directed=False):
            import networkx as nx
            assert not directed
            self.g = nx.Graph()

        def add_vertex(self, n):
            start = self.g.number_of_nodes()
            self.g.add_nodes_from(range(start, start + n))

        def add_edge_list(self, edge_list):
            for a, b in edge_list:
                assert not self.g.has_edge(a, b), "duplicate edge: graph-tool would keep both"
                self.g.add_edge(a, b)

        def vertices(self):
            return iter(self.g.nodes())

        def edges(self):
            return iter(self.g.edges())

    @staticmethod
    def label_components(g):
        import networkx as nx
        sizes = [len(c) for c in nx.connected_components(g.g)]
        return None, sizes

    @staticmethod
    def global_clustering(g):
        import networkx as nx
        triangles = sum(nx.triangles(g.g).values()) // 3
        triples = sum(d * (d - 1) // 2 for _, d in g.g.degree())
        return (3 * triangles / triples if triples > 0 else float("nan"), 0.0)


class _Tqdm:
    def __init__(self, *a, **kw):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def update(self, k=1):
        pass


def reference_namespace(record):
    import pandas as pd
    ns = {"np": np, "pd": pd, "gt": _FakeGt, "tqdm": _Tqdm, "os": os, "sys": sys, "betweenness_sample_default": 100}
    extract_functions(os.path.join(REF, "PopPUNK", "network.py"),
                      ["construct_network_from_df", "construct_network_from_edge_list", "networkSummary"], ns)
    extract_functions(os.path.join(REF, "PopPUNK", "refine.py"), ["growNetwork"], ns)
    summary = ns["networkSummary"]

    def recording_summary(G, *a, **kw):
        out = summary(G, *a, **kw)
        record.append(out[0])
        return out
    ns["networkSummary"] = recording_summary
    return ns


def clustered_distances(n, n_clusters, seed):
    """condensed float32 [n(n-1)/2, 2]: small core / accessory distances inside a cluster, larger ones between"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, n_clusters, n)
    ii, jj = np.triu_indices(n, 1)
    same = lab[ii] == lab[jj]
    core = np.where(same, rng.uniform(0.0, 0.02, ii.size), rng.uniform(0.01, 0.05, ii.size))
    acc = core * rng.uniform(2.0, 4.0, ii.size) + rng.uniform(0.0, 0.02, ii.size)
    return np.stack([core, acc], axis=1).astype(np.float32)


def stats_per_offset(i, j, idx, n, n_off):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(n))
    out = np.zeros((n_off, 4), dtype=np.int64)
    for t in range(n_off):
        sel = idx == t
        g.add_edges_from(zip(i[sel].tolist(), j[sel].tolist()))
        out[t] = (g.number_of_edges(), nx.number_connected_components(g), sum(nx.triangles(g).values()) // 3,
                  sum(d * (d - 1) // 2 for _, d in g.degree()))
    return out


def run_case(i, j, idx, n):
    record = []
    ns = reference_namespace(record)
    names = ["s%d" % k for k in range(n)]
    n_off = int(idx.max()) + 1
    scores = ns["growNetwork"](names, i.tolist(), j.tolist(), idx.tolist(), list(range(n_off)))
    present = np.unique(idx)
    assert len(record) == present.size
    return {"i": i, "j": j, "idx": idx, "n": np.int64(n), "n_off": np.int64(n_off),
            "stats": stats_per_offset(i, j, idx, n, n_off), "present": present.astype(np.int64),
            "metrics": np.array(record, dtype=np.float64), "scores": np.array(scores, dtype=np.float64)}


def main():
    from oracle import oracle
    out = {}
    cases = []

    def add(name, res):
        cases.append(name)
        for k, v in res.items():
            out["%s_%s" % (name, k)] = v

    d = clustered_distances(300, 12, 1)
    x1, y1 = float(np.median(d[:, 0])), float(np.median(d[:, 1]))
    offs = np.linspace(0.0, float(np.hypot(x1, y1)), 40)
    i, j, o = oracle.threshold_iterate_1d(d, offs, 2, 0.0, 0.0, x1, y1)
    add("sweep1d", run_case(i, j, o, 300))
    out.update(sweep1d_dist=d, sweep1d_offsets=offs, sweep1d_line=np.array([0.0, 0.0, x1, y1]))

    d = clustered_distances(200, 8, 2)
    xm = np.linspace(0.002, float(np.quantile(d[:, 0], 0.3)), 20).astype(np.float32)
    ym = float(np.quantile(d[:, 1], 0.3))
    i, j, o = oracle.threshold_iterate_2d(d, xm, ym)
    add("sweep2d", run_case(i, j, o, 200))
    out.update(sweep2d_dist=d, sweep2d_xmax=xm, sweep2d_ymax=np.float64(ym))

    d = clustered_distances(120, 6, 3)
    x1, y1 = float(np.median(d[:, 0])), float(np.median(d[:, 1]))
    i, j, o = oracle.threshold_iterate_1d(d, np.linspace(0.0, float(np.hypot(x1, y1)) * 0.8, 30), 2, 0.0, 0.0, x1, y1)
    keep = ~np.isin(o, [3, 4, 5, 9, 17])
    add("holes", run_case(i[keep], j[keep], o[keep], 120))
    keep = o >= 7
    add("late", run_case(i[keep], j[keep], o[keep], 120))

    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "network_sweep.npz")
    np.savez_compressed(path, **out)
    for c in cases:
        print(c, "n", int(out[c + "_n"]), "edges", out[c + "_i"].size, "n_off", int(out[c + "_n_off"]),
              "present", out[c + "_present"].size, "scores", out[c + "_scores"].size)


if __name__ == "__main__":
    main()
