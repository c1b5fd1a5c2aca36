"""Neighbour joining on the host side (poppunk_amd/trees.py): two restatements of the join loop,
the join record -> tree -> Newick path, midpoint rooting and the small and deep cases.  CPU only.

nj_same_rule restates the rule the device runs (ppk_nj_dev, include/ppk.h): row sums kept by the O(1) update.
nj_biopython_form restates Biopython's DistanceTreeConstructor.nj as recalled: row sums recomputed sequentially at
every join.  Both return the device's record layout, (join int64 [n-1, 2], len float64 [n-1, 2])."""
import math
import sys

import numpy as np
import pytest

from poppunk_amd import trees


def _symmetric(D):
    """float64 symmetric matrix of the strictly lower triangle of D (float32 values), zero diagonal."""
    A = np.asarray(D, dtype=np.float32).astype(np.float64)
    n = A.shape[0]
    low = np.tri(n, n, -1, dtype=bool)
    M = np.where(low, A, A.T)
    M[np.arange(n), np.arange(n)] = 0.0
    return M


def _nj(D, rowsums):
    M = _symmetric(D)
    n = M.shape[0]
    join = np.zeros((max(n - 1, 0), 2), dtype=np.int64)
    lens = np.zeros((max(n - 1, 0), 2), dtype=np.float64)
    if n < 2:
        return join, lens
    ids = np.arange(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    S = np.zeros(n)
    for j in range(n):                      # ascending columns from +0.0
        S = S + M[:, j]
    r, t = n, 0
    while r > 2:
        act = np.flatnonzero(alive)
        sub = M[np.ix_(act, act)]
        if rowsums == "same":
            nd = S[act] / (r - 2)
        else:
            s = np.zeros(r)
            for j in range(r):
                s = s + sub[:, j]
            nd = s / (r - 2)
        Q = (sub - nd[:, None]) - nd[None, :]
        Q[np.triu_indices(r)] = np.inf
        ia, ib = divmod(int(np.argmin(Q)), r)      # the first minimum in row-major order: least a, then b
        a, b = act[ia], act[ib]
        dab = M[a, b]
        la = ((dab + nd[ia]) - nd[ib]) / 2.0
        join[t] = (ids[a], ids[b])
        lens[t] = (la, dab - la)
        k = act[(act != a) & (act != b)]
        dak, dbk = M[a, k], M[b, k]
        dn = ((dak + dbk) - dab) / 2.0
        if rowsums == "same":
            S[k] = ((S[k] - dak) - dbk) + dn
            S[b] = ((S[a] + S[b]) - float(r) * dab) / 2.0
        M[b, k] = dn
        M[k, b] = dn
        ids[b] = n + t
        alive[a] = False
        r, t = r - 1, t + 1
    p0, p1 = np.flatnonzero(alive)
    join[n - 2] = (ids[p1], ids[p0])
    lens[n - 2] = (M[p1, p0], M[p1, p0])
    return join, lens


def nj_same_rule(D):
    return _nj(D, "same")


def nj_biopython_form(D):
    return _nj(D, "biopython")


def textbook():
    d = {("a", "b"): 5, ("a", "c"): 9, ("a", "d"): 9, ("a", "e"): 8, ("b", "c"): 10, ("b", "d"): 10, ("b", "e"): 9,
         ("c", "d"): 8, ("c", "e"): 7, ("d", "e"): 3}
    names = "abcde"
    D = np.zeros((5, 5), dtype=np.float32)
    for (x, y), v in d.items():
        D[names.index(x), names.index(y)] = D[names.index(y), names.index(x)] = v
    return D


def parse_newick(s):
    """(names, parent, length) of a Newick string, iteratively; unnamed nodes get names None."""
    s = s.strip()
    assert s.endswith(";")
    s = s[:-1]
    names, parent, length = [], [], []
    stack, cur, i = [], None, 0

    def new(par):
        names.append(None)
        parent.append(par)
        length.append(0.0)
        return len(names) - 1
    root = new(-1)
    node = root
    while i < len(s):
        ch = s[i]
        if ch == "(":
            stack.append(node)
            node = new(node)
            i += 1
        elif ch == ",":
            node = new(stack[-1])
            i += 1
        elif ch == ")":
            node = stack.pop()
            i += 1
        else:
            j = i
            while j < len(s) and s[j] not in "(),":
                j += 1
            tok = s[i:j]
            name, _, ln = tok.partition(":")
            names[node] = name or None
            length[node] = float(ln) if ln else 0.0
            i = j
    return names, parent, length


def patristic_from_parent(parent, length, leaves):
    """All-pairs path lengths between the given nodes of a parent-array tree."""
    def to_root(v):
        out = {}
        d = 0.0
        while v != -1:
            out[v] = d
            d += length[v] if parent[v] != -1 else 0.0
            v = parent[v]
        return out
    paths = [to_root(v) for v in leaves]
    n = len(leaves)
    P = np.zeros((n, n))
    for x in range(n):
        for y in range(x + 1, n):
            common = min((px + paths[y][v], v) for v, px in paths[x].items() if v in paths[y])
            P[x, y] = P[y, x] = common[0]
    return P


def tree_patristic(t):
    par = list(t.parent)
    ln = [0.0 if x is None else x for x in t.length]
    return patristic_from_parent(par, ln, list(range(t.n_leaves)))


@pytest.mark.parametrize("restate", [nj_same_rule, nj_biopython_form])
def test_textbook_five_taxa(restate):
    join, lens = restate(textbook())
    # a=0 b=1 c=2 d=3 e=4; u=5 (a,b), v=6 (c,u), w=7 (d,v)
    assert join.tolist() == [[1, 0], [2, 5], [3, 6], [4, 7]]
    want = [[3, 2], [4, 3], [2, 2], [1, 1]]
    np.testing.assert_allclose(lens, want, rtol=0, atol=1e-12)


def test_all_equal_ties_join_first_pair():
    D = np.ones((4, 4), dtype=np.float32)
    for restate in (nj_same_rule, nj_biopython_form):
        join, _ = restate(D)
        assert join[0].tolist() == [1, 0]
        assert join[1].tolist() == [2, 4]


def test_record_to_newick_keeps_patristic_distances():
    rng = np.random.default_rng(7)
    n = 12
    X = rng.random((n, 3))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    join, lens = nj_same_rule(D)
    unrooted = trees.tree_from_joins(join, lens, n)
    want = tree_patristic(unrooted)
    labels = ["s%d" % i for i in range(n)]
    s = trees.nj_newick(join, lens, labels)
    names, parent, length = parse_newick(s)
    leaves = [names.index(lab) for lab in labels]
    got = patristic_from_parent(parent, length, leaves)
    # %1.5f per branch: at most 5e-6 per edge on a path of fewer than 2n edges
    np.testing.assert_allclose(got, want, rtol=0, atol=2 * n * 5e-6)
    assert s.count("Inner") == n - 2 and s.endswith(";\n")


def _star_tree(lengths, children_of=None):
    t = trees.Tree(len(lengths))
    for i, ln in enumerate(lengths):
        t.length[i] = ln
    return t


def test_midpoint_on_an_edge():
    t = trees.Tree(3)
    t.length[:3] = [1.0, 1.0, 4.0]
    v = t.add_node([0, 1], "Inner1")
    t.length[v] = 1.0
    t.root = t.add_node([v, 2], "Inner2")
    trees.root_at_midpoint(t)
    assert trees.newick(t, ["A", "B", "C"]) == "(C:3.00000,(A:1.00000,B:1.00000)Inner1:2.00000):0.00000;\n"


def test_midpoint_exactly_on_a_node():
    t = trees.Tree(3)
    t.length[:3] = [1.0, 1.0, 1.0]
    t.root = t.add_node([0, 1, 2], "Inner1")
    trees.root_at_midpoint(t)
    assert trees.newick(t, ["A", "B", "C"]) == "((A:1.00000,C:1.00000)Inner1:0.00000,B:1.00000):0.00000;\n"


def test_midpoint_deep_side_and_reversed_path():
    # ((A:1,B:1)Inner1:1,(C:1,D:7)Inner2:1)Inner3 as an NJ root with a third child E:1: longest path D..A (or B)
    t = trees.Tree(5)
    t.length[:5] = [1.0, 1.0, 1.0, 7.0, 1.0]
    i1 = t.add_node([0, 1], "Inner1")
    i2 = t.add_node([2, 3], "Inner2")
    t.length[i1] = t.length[i2] = 1.0
    t.root = t.add_node([i1, i2, 4], "Inner3")
    trees.root_at_midpoint(t)
    # path D(7) Inner2(1) Inner3(1) Inner1(1) A: 10, midpoint 5 from D on D's own branch
    assert trees.newick(t, list("ABCDE")) == \
        "(D:5.00000,(((A:1.00000,B:1.00000)Inner1:1.00000,E:1.00000)Inner3:1.00000,C:1.00000)Inner2:2.00000)" \
        ":0.00000;\n"


def test_small_n():
    assert [x.shape for x in nj_same_rule(np.zeros((1, 1), np.float32))] == [(0, 2), (0, 2)]
    t = trees.tree_from_joins(np.zeros((0, 2)), np.zeros((0, 2)), 1)
    assert trees.newick(trees.root_at_midpoint(t), ["A"]) == "A:0.00000;\n"

    D2 = np.array([[0, 3], [3, 0]], np.float32)
    join, lens = nj_same_rule(D2)
    assert join.tolist() == [[1, 0]] and lens.tolist() == [[3.0, 3.0]]
    assert trees.nj_newick(join, lens, ["A", "B"]) == "(B:1.50000,A:1.50000):0.00000;\n"

    D3 = np.array([[0, 2, 4], [2, 0, 6], [4, 6, 0]], np.float32)
    for restate in (nj_same_rule, nj_biopython_form):
        join, lens = restate(D3)
        assert join.tolist() == [[1, 0], [2, 3]]
        assert lens.tolist() == [[2.0, 0.0], [4.0, 4.0]]
    t = trees.tree_from_joins(join, lens, 3)
    np.testing.assert_array_equal(tree_patristic(t), _symmetric(D3))


def test_labels_quoted_as_the_reference_strips_them():
    t = trees.Tree(2)
    t.length[:2] = [1.0, 1.0]
    t.root = t.add_node([0, 1], "Inner")
    assert trees.newick(t, ["it's", "a b"]) == "(it\\s:1.00000,a b:1.00000)Inner:0.00000;\n"


def test_deep_caterpillar_is_written_iteratively():
    n = 100_000
    join = np.zeros((n - 1, 2), dtype=np.int64)
    join[0] = (1, 0)
    for t in range(1, n - 2):
        join[t] = (t + 1, n + t - 1)
    join[n - 2] = (n - 1, 2 * n - 3)
    lens = np.ones((n - 1, 2))
    limit = sys.getrecursionlimit()
    labels = ["x%d" % i for i in range(n)]
    s = trees.nj_newick(join, lens, labels)
    assert sys.getrecursionlimit() == limit
    assert s.count("(") == s.count(")") and s.count("(") == n - 1
    assert s.endswith(":0.00000;\n") and "x99999:" in s


def test_generate_nj_tree_signature_and_write_tree(tmp_path):
    import inspect
    sig = inspect.signature(trees.generate_nj_tree)
    assert list(sig.parameters) == ["coreMat", "seqLabels", "outPrefix", "tmp", "rapidnj", "threads"]
    prefix = str(tmp_path / "out")
    (tmp_path / "out").mkdir()
    trees.write_tree("(A:1.00000,B:1.00000):0.00000;\n", prefix, "_core_NJ.nwk", False)
    path = tmp_path / "out" / "out_core_NJ.nwk"
    assert path.read_text().startswith("(A:")
    trees.write_tree("X", prefix, "_core_NJ.nwk", False)
    assert path.read_text().startswith("(A:")
    trees.write_tree("X", prefix, "_core_NJ.nwk", True)
    assert path.read_text() == "X"


def test_restatements_agree_on_topology_where_margins_are_clear():
    rng = np.random.default_rng(3)
    X = rng.random((40, 4))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    a, la = nj_same_rule(D)
    b, lb = nj_biopython_form(D)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(la, lb, rtol=0, atol=1e-9)
    assert math.isfinite(float(la.sum()))
