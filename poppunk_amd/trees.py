"""Neighbour-joining trees for poppunk_visualise (PopPUNK/trees.py): generate_nj_tree and write_tree.

The join loop runs on the device (engine.nj_dev); everything after it is host code in O(n) and
iterative, so a caterpillar of any size is written without recursion:
  - tree_from_joins: the join record -> the unrooted tree Biopython's DistanceTreeConstructor.nj builds, as recalled
    (inner nodes Inner1, Inner2, ... in join order with children [a, b]; the last inner node is the root and takes
    the final edge's other node as a third child; n = 2 gives a root "Inner" whose children have length D/2 each);
  - root_at_midpoint: Tree.root_at_midpoint;
  - newick: Phylo.write(tree, ..., "newick") with tree_as_string's quote stripping.
String-for-string equality with Biopython's output is unverified (tools/pin_nj.py checks it where Biopython is
installed); the tree, its branch lengths and its root position are what this module is held to."""
import math
import os
import re
import sys

import numpy as np


class Tree:
    """A rooted tree on node ids 0 .. len(children) - 1: leaves 0 .. n_leaves - 1 name samples.  children[v] is an
    ordered list, length[v] the branch above v (None: no branch), name[v] an inner node's label or None."""

    def __init__(self, n_leaves):
        self.n_leaves = n_leaves
        self.children = [[] for _ in range(n_leaves)]
        self.parent = [-1] * n_leaves
        self.length = [None] * n_leaves
        self.name = [None] * n_leaves
        self.root = 0 if n_leaves else -1

    def add_node(self, children, name=None):
        v = len(self.children)
        self.children.append(list(children))
        self.parent.append(-1)
        self.length.append(None)
        self.name.append(name)
        for c in children:
            self.parent[c] = v
        return v


def tree_from_joins(join, lens, n):
    """The unrooted NJ tree of a join record (engine.nj_dev / ppk_nj_dev layout, host arrays)."""
    join = np.asarray(join, dtype=np.int64).reshape(-1, 2)
    lens = np.asarray(lens, dtype=np.float64).reshape(-1, 2)
    n = int(n)
    if n < 1 or len(join) != n - 1 or len(lens) != n - 1:
        raise ValueError("a join record of n samples has n - 1 rows")
    t = Tree(n)
    if n == 1:
        return t
    if n == 2:
        d = float(lens[0, 0])
        x1, x0 = int(join[0, 0]), int(join[0, 1])
        t.length[x1] = d / 2.0
        t.length[x0] = d - t.length[x1]
        t.root = t.add_node([x1, x0], "Inner")
        return t
    for k in range(n - 2):
        a, b = int(join[k, 0]), int(join[k, 1])
        if not (0 <= a < n + k and 0 <= b < n + k) or t.parent[a] != -1 or t.parent[b] != -1:
            raise ValueError("join %d does not join two free nodes" % k)
        t.length[a] = float(lens[k, 0])
        t.length[b] = float(lens[k, 1])
        t.add_node([a, b], "Inner%d" % (k + 1))
    last = 2 * n - 3
    x1, x0 = int(join[n - 2, 0]), int(join[n - 2, 1])
    if last not in (x1, x0):
        raise ValueError("the final edge does not end at the last inner node")
    other = x0 if x1 == last else x1
    if t.parent[other] != -1 or other == last:
        raise ValueError("the final edge's other end is not a free node")
    t.length[last] = 0.0
    t.length[other] = float(lens[n - 2, 0])
    t.children[last].append(other)
    t.parent[other] = last
    t.root = last
    return t


def _postorder(t):
    """Every node reachable from the root, children before their parent."""
    out, stack = [], [t.root]
    while stack:
        v = stack.pop()
        out.append(v)
        stack.extend(t.children[v])
    return out[::-1]


def root_at_midpoint(t):
    """Root the tree at the midpoint of its longest tip-to-tip path (Tree.root_at_midpoint), in place; returns t.

    The longest path: for every node v, its two children c maximising length[c] + (the longest path from c down to
    a tip); a node with the strictly largest sum over all nodes, in post-order (children in their order, the first
    of equal values kept) names the path x ... v ... y, x on the side of the larger (or first) child.  Walking from x
    towards y, remaining = total / 2 loses each edge's length; the root goes on the first edge where remaining
    becomes negative (strictly), -remaining of the edge on y's side and the rest on x's side.  A midpoint exactly on
    a node therefore sits on the next edge, with a zero-length branch to that node; with no such edge (a path of
    total length <= 0) the root takes the last edge, all of it on x's side.  The new root's children are [x side,
    y side]; each node whose parent changes takes its old parent as its first child, and an old root left with one
    child is spliced out, its branch added to the child's."""
    if len(t.children) < 2 or t.n_leaves < 2:
        return t
    down, tip = {}, {}
    best, where = -math.inf, None
    for v in _postorder(t):
        ch = t.children[v]
        if not ch:
            down[v], tip[v] = 0.0, v
            continue
        vals = [t.length[c] + down[c] for c in ch]
        i1 = max(range(len(ch)), key=lambda i: (vals[i], -i))
        down[v], tip[v] = vals[i1], tip[ch[i1]]
        if len(ch) > 1:
            i2 = max((i for i in range(len(ch)) if i != i1), key=lambda i: (vals[i], -i))
            if vals[i1] + vals[i2] > best:
                best, where = vals[i1] + vals[i2], (v, ch[i1], ch[i2])
    if where is None:
        return t
    v, c1, c2 = where
    x, y = tip[c1], tip[c2]
    up = [x]
    while up[-1] != v:
        up.append(t.parent[up[-1]])
    dn = [y]
    while dn[-1] != v:
        dn.append(t.parent[dn[-1]])
    path = up + dn[-2::-1]
    remaining = 0.5 * best
    split = None
    for i in range(1, len(path)):
        u, w = path[i - 1], path[i]
        ln = t.length[u] if t.parent[u] == w else t.length[w]
        remaining -= ln
        if remaining < 0:
            split = (u, w, ln + remaining, -remaining)
            break
    if split is None:
        u, w = path[-2], path[-1]
        ln = t.length[u] if t.parent[u] == w else t.length[w]
        split = (u, w, ln, 0.0)
    u, w, lu, lw = split
    _reroot(t, u, w, lu, lw)
    return t


def _reroot(t, u, w, lu, lw):
    """A new root on the edge (u, w): branches lu to u, lw to w; children [u, w]."""
    p, c = (w, u) if t.parent[u] == w else (u, w)
    old_root = t.root
    t.children[p].remove(c)
    r = t.add_node([], None)
    t.children[r] = [u, w]
    t.length[c] = lu if c == u else lw
    # reverse the path from p up to the old root: each node takes its old parent as its first child
    prev_len = t.length[p]
    t.length[p] = lu if p == u else lw
    cur, up = p, t.parent[p]
    t.parent[u], t.parent[w] = r, r
    while up != -1:
        nxt = t.parent[up]
        t.children[up].remove(cur)
        t.children[cur].insert(0, up)
        t.parent[up] = cur
        prev_len, t.length[up] = t.length[up], prev_len
        cur, up = up, nxt
    t.root = r
    if old_root != r and len(t.children[old_root]) == 1:
        only, par = t.children[old_root][0], t.parent[old_root]
        t.length[only] = (t.length[only] or 0.0) + (t.length[old_root] or 0.0)
        t.children[par][t.children[par].index(old_root)] = only
        t.parent[only] = par
        t.children[old_root] = []
        t.parent[old_root] = -1


_UNQUOTED = re.compile(r"[^\s\(\)\[\]\'\:\;\,]+")


def _label(s):
    """A name as Phylo's Newick writer quotes it, after tree_as_string removes the single quotes."""
    s = "" if s is None else str(s)
    m = _UNQUOTED.match(s)
    if s and (not m or m.end() < len(s)):
        s = s.replace("\\", "\\\\").replace("'", "\\'")
    return s.replace("'", "")


def newick(t, labels):
    """Phylo.write(tree, ..., "newick") then tree_as_string's quote stripping, iteratively: "(c1,c2,...)name:len"
    per node in child order, lengths "%1.5f" (none written as 0.00000), leaves named by labels, ";\\n" at the end."""
    if t.root < 0:
        raise ValueError("empty tree")
    out = []
    stack = [(t.root, 0)]
    while stack:
        v, i = stack.pop()
        ch = t.children[v]
        if not ch:
            out.append(_label(labels[v]) + ":%1.5f" % (t.length[v] or 0.0))
            continue
        if i == 0:
            out.append("(")
        elif i < len(ch):
            out.append(",")
        if i < len(ch):
            stack.append((v, i + 1))
            stack.append((ch[i], 0))
        else:
            out.append(")" + _label(t.name[v]) + ":%1.5f" % (t.length[v] or 0.0))
    return "".join(out) + ";\n"


def nj_newick(join, lens, seqLabels):
    """The midpoint-rooted Newick string of a join record."""
    t = tree_from_joins(join, lens, len(seqLabels))
    root_at_midpoint(t)
    return newick(t, list(seqLabels))


def generate_nj_tree(coreMat, seqLabels, outPrefix, tmp=None, rapidnj=None, threads=1):
    """Neighbour-joining tree of core distances (PopPUNK/trees.py:157-197), midpoint rooted, as a Newick string.

    coreMat: the n x n core distances, numpy or a float32 CUDA tensor (read in place; only the strictly lower
    triangle is read), or the resident long form as engine.nj_dev takes it.  The device join loop
    (engine.nj_dev, Biopython's nj rule) replaces both of the reference's branches, so tmp, rapidnj and threads are
    accepted for its signature and ignored; outPrefix is not written to either."""
    from . import engine
    sys.stderr.write("Building phylogeny\n")
    if hasattr(coreMat, "is_cuda") and coreMat.is_cuda:
        join, lens = engine.nj_dev(coreMat)
        join, lens = join.cpu().numpy(), lens.cpu().numpy()
    else:
        join, lens = engine.nj(np.asarray(coreMat, dtype=np.float32))
    return nj_newick(join, lens, list(seqLabels))


def write_tree(tree, prefix, suffix, overwrite):
    """Prints a Newick-formatted string to prefix/basename(prefix) + suffix (PopPUNK/trees.py:94-112)."""
    tree_filename = prefix + "/" + os.path.basename(prefix) + suffix
    if overwrite or not os.path.isfile(tree_filename):
        with open(tree_filename, 'w') as tree_file:
            tree_file.write(tree)
    else:
        sys.stderr.write("Unable to write phylogeny to " + tree_filename + "\n")
