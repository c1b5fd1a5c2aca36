#!/usr/bin/env python3
"""Generates tests/golden/mst.npz: generate_minimum_spanning_tree as the reference computes it.

Run in the BUILD container only (needs the reference checkout); the fixture it writes is data and is committed, the
reference is not.  PopPUNK/network.py's generate_minimum_spanning_tree is pulled out with make_golden_network.py's
`ast` helper and run unmodified (from_cugraph=False, the graph-tool branch) on a small stand-in for graph-tool (not in
this image), a list-backed undirected multigraph:
  Graph, add_vertex, add_edge_list(list, eprops=[p]) (columns past the second fill the property; without eprops they
  are ignored and the new edges' property values are 0), new_ep, edge_properties / ep, get_vertices,
  get_out_degrees, get_all_edges(v, [p]) (every edge at v in insertion order, as rows [v, other, p]), get_edges([p]),
  GraphView(g, efilt=...) / GraphView(g, vfilt=...), Graph(view, prune=True), label_components (components numbered
  by smallest vertex) and min_spanning_tree: Kruskal over a stable sort on the weight alone, so among equal weights
  the earlier edge wins.  That tie rule is the stand-in's; graph-tool's (boost Kruskal's priority queue) is
  implementation-defined.  The new-edge property value 0 is also the stand-in's reading, unverified.

The forest spans G's components, so G never has an edge between two seeds and every case takes the max_weight
fallback of network.py:1808-1811; the branch that takes G's seed-to-seed edges is unreachable through this function
(tests/test_mst_host.py drives it through the host step directly).

Arrays (prefix `<case>_`; `cases` lists them): edges int64 [m, 2], n, weights float64 [m] (distinct float32 values;
the tree is unique), out_edges int64 [k, 2] and out_weights float64 [k] (the returned graph's edges in edge order and
their weight property), seeds int64 (in the order the reference's set iterates them), n_components (of the forest).
Cases: connected (one component, no seed step), two (two components: the seed link is unique), multi (five components
with isolated vertices, ids scattered so the set does not iterate in sorted order), parallel (both orientations and
parallel edges of each pair, as a kNN list has them; three components).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_network as mgn  # noqa: E402


class _Prop:
    def __init__(self, g, values=None):
        self.g = g
        self.v = list(values) if values is not None else [0.0] * len(g.e)

    @property
    def a(self):
        return np.asarray(self.v, dtype=np.float64)

    def __getitem__(self, k):
        return self.v[k]


class _Graph:
    def __init__(self, src=None, directed=False, prune=False):
        assert not directed
        self.n, self.e, self.edge_properties = 0, [], {}
        if src is not None:                   # Graph(GraphView(g, efilt=f), prune=True): the kept edges, in order
            keep = [k for k in range(len(src.e)) if src.efilt[k]]
            self.n = src.n
            self.e = [src.e[k] for k in keep]
            for name, p in src.edge_properties.items():
                self.edge_properties[name] = _Prop(self, [p.v[k] for k in keep])

    @property
    def ep(self):
        return self.edge_properties

    def add_vertex(self, k):
        self.n += int(k)

    def new_ep(self, kind):
        assert kind == "float"
        return _Prop(self)

    def add_edge_list(self, edge_list, eprops=None):
        for row in edge_list:
            a, b = int(row[0]), int(row[1])
            self.n = max(self.n, a + 1, b + 1)
            self.e.append((a, b))
            for p in self.edge_properties.values():
                p.v.append(0.0)
            for q, p in enumerate(eprops or []):
                if p not in self.edge_properties.values():
                    p.v.append(float(row[2 + q]))
                else:
                    p.v[-1] = float(row[2 + q])

    def get_vertices(self):
        return np.arange(self.n)

    def get_all_edges(self, v, eprops):
        rows = []
        for k, (a, b) in enumerate(self.e):
            if a == v or b == v:
                rows.append([v, b if a == v else a] + [p.v[k] for p in eprops])
        return np.array(rows, dtype=np.float64).reshape(-1, 2 + len(eprops))

    def get_edges(self, eprops):
        keep = [k for k in range(len(self.e)) if getattr(self, "efilt", None) is None or self.efilt[k]]
        return np.array([[self.e[k][0], self.e[k][1]] + [p.v[k] for p in eprops] for k in keep],
                        dtype=np.float64).reshape(-1, 2 + len(eprops))


class _VertexView:
    def __init__(self, g, vfilt):
        self.g, self.keep = g, np.flatnonzero(np.asarray(vfilt))

    def get_vertices(self):
        return self.keep.copy()

    def get_out_degrees(self, vs):
        inside = set(self.keep.tolist())
        deg = {int(v): 0 for v in vs}
        for a, b in self.g.e:
            if a in inside and b in inside:
                deg[a] += 1
                deg[b] += 1
        return np.array([deg[int(v)] for v in vs])


class _Gt:
    Graph = _Graph

    @staticmethod
    def GraphView(g, efilt=None, vfilt=None):
        if vfilt is not None:
            return _VertexView(g, vfilt)
        view = _Graph.__new__(_Graph)
        view.n, view.e, view.edge_properties, view.efilt = g.n, g.e, g.edge_properties, list(efilt)
        return view

    @staticmethod
    def min_spanning_tree(g, weights):
        order = sorted(range(len(g.e)), key=lambda k: weights.v[k])
        parent = list(range(g.n))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        keep = [False] * len(g.e)
        for k in order:
            a, b = find(g.e[k][0]), find(g.e[k][1])
            if a != b:
                parent[max(a, b)] = min(a, b)
                keep[k] = True
        return keep

    @staticmethod
    def label_components(g):
        parent = list(range(g.n))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for a, b in g.e:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        roots = [find(v) for v in range(g.n)]
        ids = {}
        for r in roots:
            ids.setdefault(r, len(ids))
        lab = np.array([ids[r] for r in roots], dtype=np.int64)
        return _Prop(g, lab), np.bincount(lab, minlength=len(ids))


def run(edges, n, weights):
    ns = {"np": np, "gt": _Gt, "sys": sys, "cugraph": None, "cudf": None}
    mgn.extract_functions(os.path.join(mgn.REF, "PopPUNK", "network.py"), ["generate_minimum_spanning_tree"], ns)
    G = _Graph()
    G.add_vertex(n)
    w = _Prop(G)
    G.add_edge_list([(int(a), int(b), float(x)) for (a, b), x in zip(edges.tolist(), weights.tolist())], eprops=[w])
    G.edge_properties["weight"] = w
    seeds = []
    real_set = set

    class _Set(real_set):                    # records the reference's seed set as it is iterated
        def __iter__(self):
            items = list(real_set.__iter__(self))
            if not seeds:
                seeds.extend(int(v) for v in items)
            return iter(items)
    ns["set"] = _Set
    out = ns["generate_minimum_spanning_tree"](G, False)
    forest = _Gt.min_spanning_tree(G, G.ep["weight"])
    n_comp = len(_Gt.label_components(_Graph(_Gt.GraphView(G, efilt=forest), prune=True))[1])
    return {"edges": edges.astype(np.int64), "n": np.int64(n), "weights": weights.astype(np.float64),
            "out_edges": np.array(out.e, dtype=np.int64).reshape(-1, 2), "out_weights": out.ep["weight"].a,
            "seeds": np.array(seeds, dtype=np.int64), "n_components": np.int64(n_comp)}


def random_case(rng, sizes, n_isolated, extra, parallel=False):
    edges, at = [], 0
    for s in sizes:
        v = list(range(at, at + s))
        at += s
        for k in range(1, s):
            edges.append((v[int(rng.integers(0, k))], v[k]))
        for _ in range(extra * s):
            a, b = rng.choice(v, 2, replace=False)
            edges.append((int(a), int(b)))
    n = at + n_isolated
    edges = np.array(edges, dtype=np.int64)
    if parallel:
        edges = np.concatenate([edges, edges[:, ::-1], edges[: len(edges) // 3]])
    perm = rng.permutation(n)
    edges = perm[edges][rng.permutation(len(edges))]
    w = rng.permutation(len(edges)).astype(np.float32) / np.float32(7) + np.float32(0.01)   # distinct float32 values
    return edges, n, w


def main():
    rng = np.random.default_rng(11)
    cases = {"connected": random_case(rng, [40], 0, 2), "two": random_case(rng, [25, 12], 0, 2),
             "multi": random_case(rng, [20, 14, 9, 5], 4, 1), "parallel": random_case(rng, [18, 10, 7], 0, 1, True)}
    out = {"cases": np.array(list(cases))}
    for name, (e, n, w) in cases.items():
        for k, v in run(e, n, w).items():
            out["%s_%s" % (name, k)] = v
        print(name, "n", n, "edges", len(e), "components", int(out[name + "_n_components"]), "seeds",
              out[name + "_seeds"].tolist(), "out", len(out[name + "_out_edges"]))
    np.savez_compressed(os.path.join(HERE, "mst.npz"), **out)


if __name__ == "__main__":
    main()
