#!/usr/bin/env python3
"""Generates tests/golden/references.npz: the reference genomes the reference's own loop picks on a few small graphs.

Run in the BUILD container only (needs the reference checkout, networkx, pandas and scipy); what it writes is data
(edge lists, flags, chosen indices, the bytes of the .refs files) and is committed, the reference is not.

Reference code executed (pulled out of PopPUNK/network.py with `ast`, as make_golden_network.py does, and run
unmodified): getCliqueRefs, cliquePrune, fastPrune, extractReferences, writeReferences, and printClusters, which
extractReferences calls -- under make_golden_clusters.py's networkx stand-in for graph-tool, extended HERE with
GraphView, Graph(view, prune=True), vertex properties, max_cliques (networkx.find_cliques), shortest_path and a serial
Pool.  networkx's clique order is NOT graph-tool's, and list(frozenset)[0] is CPython's: the indices recorded are a
choice the reference's loop can make, not the one graph-tool makes.  No test compares our count with these.

references.npz, for case k = 0 ..: n_k, edges_k int64 [m, 2], existing_k uint8 [n], fast_k, chosen_k (sorted int64
indices), refs_file_k (the .refs file's bytes as uint8); `cases`, their count.  Names are "s%03d" % index.
"""
import contextlib
import io
import os
import sys
import tempfile
from collections import defaultdict
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden_clusters as mgc         # noqa: E402
import make_golden_network as mgn          # noqa: E402
import refs_model as rm                    # noqa: E402

REF = mgn.REF


class _View:
    """GraphView(base, vfilt): vfilt holds one flag per vertex of the root graph (a property or an array), or one
    per vertex of `base` in its iteration order (getCliqueRefs' list)"""

    def __init__(self, base, vfilt):
        self.root = base.root
        nodes = base.nodes
        flags = list(vfilt)
        if len(flags) == self.root.g.number_of_nodes():
            self.nodes = [v for v in nodes if flags[v]]
        else:
            assert len(flags) == len(nodes)
            self.nodes = [v for v, f in zip(nodes, flags) if f]
        self.g = self.root.g.subgraph(self.nodes)

    def vertices(self):
        return iter(self.nodes)

    def num_vertices(self):
        return len(self.nodes)

    def get_vertices(self):
        return np.asarray(self.nodes, dtype=np.int64)


class _Graph(mgc._Gt.Graph):
    def __init__(self, src=None, directed=False, prune=False):
        super().__init__(directed)
        if src is not None:                # Graph(view, prune=True): the view's vertices renumbered by rank
            assert prune
            rank = {v: k for k, v in enumerate(src.nodes)}
            self.add_vertex(len(rank))
            self.add_edge_list(sorted((min(rank[a], rank[b]), max(rank[a], rank[b])) for a, b in src.g.edges()))

    root = property(lambda self: self)
    nodes = property(lambda self: sorted(self.g.nodes()))

    def num_vertices(self):
        return self.g.number_of_nodes()

    def get_vertices(self):
        return np.asarray(self.nodes, dtype=np.int64)

    def new_vertex_property(self, kind):
        assert kind == 'bool'
        return [False] * self.g.number_of_nodes()


class _Gt(mgc._Gt):
    Graph = _Graph
    GraphView = _View

    @staticmethod
    def openmp_enabled():
        return False

    @staticmethod
    def max_cliques(g):
        import networkx as nx
        return iter(nx.find_cliques(g.g))

    @staticmethod
    def shortest_path(g, a, b):
        import networkx as nx
        return nx.shortest_path(g.g, int(a), int(b)), None


class _Pool:
    def __init__(self, processes=1):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def map(self, fn, items):
        return [fn(x) for x in items]


def reference_namespace():
    ns = mgc.reference_namespace()
    ns.update({"gt": _Gt, "Pool": _Pool, "partial": partial, "defaultdict": defaultdict, "FAST_REF_SUBSAMPLE": None,
               "FAST_REF_MERGE_SUBSAMPLE": None})
    import ast
    path = os.path.join(REF, "PopPUNK", "network.py")
    for node in ast.parse(open(path).read()).body:        # the two module constants fastPrune reads
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("FAST_REF_SUBSAMPLE",
                                                                                  "FAST_REF_MERGE_SUBSAMPLE"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    assert ns["FAST_REF_SUBSAMPLE"] == 10 and ns["FAST_REF_MERGE_SUBSAMPLE"] == 3, "the reference has moved"
    mgn.extract_functions(path, ["getCliqueRefs", "cliquePrune", "fastPrune", "extractReferences", "writeReferences"], ns)
    return ns


def cases():
    d, dn = rm.dumbbell()
    mixed = rm.shifted([(rm.path(40), 40), (rm.star(30), 31), (rm.clique(12), 12), ([], 3), ([(0, 1)], 2),
                        (rm.random_graph(66, 0.5, 1), 66)])
    withref = rm.planted(240, 4, 0.5, 2, 21)
    existing = np.zeros(240, dtype=np.uint8)
    existing[[5, 77, 130, 131]] = 1
    return [(*rm.planted(300, 5, 0.3, 3, 11), None, False),
            (*rm.planted(200, 4, 0.6, 0, 12), None, False),
            (np.asarray(d, dtype=np.int64), dn, None, False),
            (*mixed, None, False),
            (*withref, existing, False),
            (*rm.planted(300, 5, 0.15, 4, 13), None, False),
            (*rm.planted(300, 5, 0.3, 3, 11), None, True)]


def main():
    ns = reference_namespace()
    out = {}
    all_cases = cases()
    for k, (edges, n, existing, fast) in enumerate(all_cases):
        edges = np.unique(np.sort(np.asarray(edges, dtype=np.int64).reshape(-1, 2), axis=1), axis=0)
        names = ["s%03d" % v for v in range(n)]
        g = _Graph()
        g.add_vertex(n)
        g.add_edge_list([tuple(e) for e in edges.tolist()])
        with tempfile.TemporaryDirectory() as tmp:
            prefix = os.path.join(tmp, "db")
            os.makedirs(prefix)
            with contextlib.redirect_stderr(io.StringIO()):
                idx, ref_names, ref_file, g_ref = ns["extractReferences"](
                    g, names, prefix, existingRefs=None if existing is None else [names[v] for v in np.flatnonzero(existing)],
                    fast_mode=fast)
            text = open(ref_file, "rb").read()
        chosen = np.asarray(sorted(int(v) for v in idx), dtype=np.int64)
        assert ref_names == [names[v] for v in chosen] and g_ref.num_vertices() == len(chosen)
        out.update({"n_%d" % k: np.int64(n), "edges_%d" % k: edges, "fast_%d" % k: np.int64(fast),
                    "existing_%d" % k: np.zeros(n, dtype=np.uint8) if existing is None else existing,
                    "chosen_%d" % k: chosen, "refs_file_%d" % k: np.frombuffer(text, dtype=np.uint8)})
        ours = rm.pick_refs(edges, n, existing, None, fast)[2]["references"]
        print("case %d: n = %d, %d edges, fast %d: the stand-in's loop picked %d, the rule %d"
              % (k, n, len(edges), fast, len(chosen), ours))
    out["cases"] = np.int64(len(all_cases))
    np.savez_compressed(os.path.join(HERE, "references.npz"), **out)


if __name__ == "__main__":
    main()
