#!/usr/bin/env python3
"""Pin kit: settle the neighbour-joining tree against the reference's generate_nj_tree.

poppunk_amd.trees restates Biopython's DistanceTreeConstructor.nj, Tree.root_at_midpoint and its Newick writer as
recalled; Biopython is not installed where this library is built.  Wherever Biopython, the reference's
PopPUNK.trees and this package with an MI355X are all importable, this script runs the reference's
generate_nj_tree(coreMat, labels, outPrefix, rapidnj=None) and poppunk_amd.trees.generate_nj_tree on the same
matrices (dyadic random, an additive tree, designed ties, synthetic core distances) and compares them AS TREES:

  - the unrooted bipartitions (sets of leaf names on either side of every edge) are equal;
  - every bipartition's branch length agrees to 1e-9 (the written lengths are %1.5f, so the comparison reads the
    reference's Phylo tree before it is written, and this package's join record);
  - the root sits on the same bipartition's edge, at the same distance to 1e-9 from either end;

and reports whether the Newick strings are equal character for character (unverified by design: child order after
rerooting and the tie rule of the longest path may differ without changing the tree).

    python tools/pin_nj.py [--device N]

Exit status 0 = every tree equal, 1 = some tree differs (the line says how), 2 = Biopython or the reference's
PopPUNK.trees not importable (nothing pinned).  It is EXPECTED to exit 2 in the build container and on the GPU box.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def matrices():
    rng = np.random.default_rng(0)
    out = []
    for n in (5, 17, 64, 200):
        A = rng.integers(0, 2048, size=(n, n)).astype(np.float32) / np.float32(1024)
        out.append(("dyadic_%d" % n, np.tril(A, -1) + np.tril(A, -1).T))
    out.append(("all_equal_30", np.full((30, 30), 0.5, dtype=np.float32) - np.eye(30, dtype=np.float32) * 0.5))
    X = rng.random((150, 4))
    out.append(("euclidean_150", np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)).astype(np.float32)))
    return out


def splits_of(edges, leaves):
    """{frozenset(side without the first leaf): length} of an unrooted tree given as (parent, child, length) edges
    over hashable node keys, a node of degree 2 (a root on an edge) merged into one edge."""
    adj = {}
    for p, c, ln in edges:
        adj.setdefault(p, []).append((c, ln))
        adj.setdefault(c, []).append((p, ln))
    first = leaves[0]
    out = {}
    seen = set()
    for p, c, ln in edges:
        # leaves below c when the edge is cut
        stack, side, vis = [c], set(), {p, c}
        while stack:
            v = stack.pop()
            if v in leaves:
                side.add(v)
            for w, _ in adj[v]:
                if w not in vis:
                    vis.add(w)
                    stack.append(w)
        if first in side:
            side = set(leaves) - side
        key = frozenset(side)
        out[key] = out.get(key, 0.0) + ln
        seen.add(key)
    return out


def reference_edges(tree):
    edges = []
    for clade in tree.find_clades(order="level"):
        for ch in clade.clades:
            edges.append((id(clade), ch.name if ch.is_terminal() else id(ch), ch.branch_length or 0.0))
    return edges


def ours_edges(t, labels):
    key = lambda v: labels[v] if v < t.n_leaves else ("node", v)   # noqa: E731
    edges = []
    for v in range(len(t.children)):
        for c in t.children[v]:
            edges.append((key(v), key(c), t.length[c] or 0.0))
    return edges


def below(t, v):
    out, stack = [], [v]
    while stack:
        x = stack.pop()
        if t.children[x]:
            stack.extend(t.children[x])
        else:
            out.append(x)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    try:
        from Bio.Phylo.TreeConstruction import DistanceMatrix, DistanceTreeConstructor
        from PopPUNK import trees as ref_trees
    except ImportError as e:
        print("pin_nj: nothing pinned (%s)" % e)
        return 2
    from poppunk_amd import engine, trees
    bad = 0
    for name, D in matrices():
        n = D.shape[0]
        labels = ["s%d" % i for i in range(n)]
        ref_str = ref_trees.generate_nj_tree(D.astype(np.float64), labels, ".", rapidnj=None)
        # the same tree before it is written (the else branch of PopPUNK/trees.py:184-190): full-precision lengths
        ref_tree = DistanceTreeConstructor().nj(DistanceMatrix(labels, [D[i, :i + 1].astype(np.float64).tolist()
                                                                        for i in range(n)]))
        ref_tree.root_at_midpoint()
        join, lens = engine.nj(D, device_id=a.device)
        ours = trees.root_at_midpoint(trees.tree_from_joins(join, lens, n))
        ours_str = trees.newick(ours, labels)
        rs, os_ = splits_of(reference_edges(ref_tree), labels), splits_of(ours_edges(ours, labels), labels)
        why = []
        if set(rs) != set(os_):
            why.append("bipartitions differ (%d vs %d, %d shared)" % (len(rs), len(os_), len(set(rs) & set(os_))))
        else:
            err = max(abs(rs[k] - os_[k]) for k in rs)
            if err > 1e-9:
                why.append("branch lengths differ by %.3g" % err)
        # root: the bipartition of the edge it sits on, and its distance to the side without the first leaf
        rr = [(frozenset(x.name for x in c.get_terminals()), c.branch_length or 0.0) for c in ref_tree.root.clades]
        oo = [(frozenset(labels[x] for x in below(ours, c)), ours.length[c] or 0.0) for c in ours.children[ours.root]]
        if len(rr) != 2 or len(oo) != 2:
            why.append("a root with %d / %d children" % (len(rr), len(oo)))
        else:
            rk = [x for x in rr if labels[0] not in x[0]][0]
            ok = [x for x in oo if labels[0] not in x[0]][0]
            if rk[0] != ok[0] or abs(rk[1] - ok[1]) > 1e-9:
                why.append("root position differs")
        print("%-16s %s; strings %s" % (name, "; ".join(why) or "equal trees",
                                        "equal" if ref_str == ours_str else "differ"))
        bad += bool(why)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
