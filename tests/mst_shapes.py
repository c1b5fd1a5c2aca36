"""Input builders for the shapes of ppk_mst.hip that random multigraphs never reach, the references
the MST tests share (a Python Kruskal under the contract's total order, scipy's labels, the multigraph generator) and a
numpy restatement of the device's Boruvka rounds.  tests/test_mst_host.py proves on the CPU what each builder claims;
tests/test_gpu_mst_shapes.py runs them on the device.  This file holds no test."""
import numpy as np


# ---- references ------------------------------------------------------------------------------------------------------
def kruskal(edges, n, w):
    """Kruskal with a stable sort on (w, min, max, index), -0.0 == +0.0: indices ascending, and scipy-style labels."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float32).astype(np.float64) + 0.0
    order = np.lexsort((np.arange(len(e)), e.max(axis=1), e.min(axis=1), w))
    parent = np.arange(n)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    keep = []
    for k in order.tolist():
        a, b = find(e[k, 0]), find(e[k, 1])
        if a != b:
            parent[max(a, b)] = min(a, b)
            keep.append(k)
    return np.array(sorted(keep), dtype=np.int64)


def scipy_labels(edges, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = np.asarray(edges).reshape(-1, 2)
    return connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)


def multigraph(rng, n, n_comp, n_edges, levels, vals=None):
    """Random multigraph: vertices split into n_comp groups plus isolated ones, edges inside groups in both
    orientations with parallel copies, weights from a few levels (many ties, 0.0 and -0.0 among them), or from the
    `levels` float32 values of `vals`."""
    groups = rng.integers(0, n_comp + 1, n)                  # group n_comp: isolated
    members = [np.flatnonzero(groups == g) for g in range(n_comp)]
    members = [m for m in members if m.size > 1]
    e = []
    for _ in range(n_edges):
        m = members[int(rng.integers(0, len(members)))]
        a, b = rng.choice(m, 2, replace=False)
        e.append((a, b))
    e = np.array(e, dtype=np.int64)
    dup = rng.random(len(e)) < 0.2
    e = np.concatenate([e, e[dup][:, ::-1], e[rng.random(len(e)) < 0.1]])
    if vals is None:
        vals = np.concatenate([[0.0, -0.0], rng.random(levels - 2)]).astype(np.float32)
    assert vals.dtype == np.float32 and len(vals) == levels
    w = vals[rng.integers(0, levels, len(e))]
    return e, w


def ceil_log2(n):
    """The least r with 2^r >= n: the device's round count and key width (at least 1 there)."""
    return int(n - 1).bit_length() if n > 1 else 0


def jump_passes(n):
    """ppk_mst_dev's compression passes per round: 16^passes >= n, made odd."""
    p = 1
    while p < 8 and 16 ** p < n:
        p += 1
    return p + 1 - (p & 1)


def shuffled(e, w, seed):
    """The same multigraph with its edges permuted and about half of them flipped: (e, w, pos), pos[k] the new index
    of edge k."""
    rng = np.random.default_rng(seed)
    p = rng.permutation(len(e))
    e2 = e[p].copy()
    flip = rng.random(len(e)) < 0.5
    e2[flip] = e2[flip][:, ::-1]
    pos = np.empty(len(e), dtype=np.int64)
    pos[p] = np.arange(len(e))
    return e2, w[p].copy(), pos


# ---- the rounds of ppk_mst.hip ---------------------------------------------------------------------------------------
def boruvka(e, w, n):
    """The rounds of ppk_mst.hip restated: edges ranked by (w + 0.0, min, max, index); each round every edge between
    two different roots lowers both roots' best rank, every root hooks along its best edge except the smaller root of
    a mutual pair, and the hook forest is compressed fully.  Returns (the tree's input indices ascending, the number
    of rounds that hooked, every such round's hook-forest depth: the longest walk along dst to a root).  The depth
    walk is O(n * depth): for n <= 10 000."""
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    m = len(e)
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64) + 0.0
    order = np.lexsort((np.arange(m), e.max(axis=1), e.min(axis=1), w64))
    eu, ev = e[order, 0], e[order, 1]
    comp = np.arange(n)
    chosen = np.zeros(m, dtype=bool)
    depths = []
    while True:
        cu, cv = comp[eu], comp[ev]
        live = np.flatnonzero(cu != cv)
        if live.size == 0:
            break
        best = np.full(n, m, dtype=np.int64)
        np.minimum.at(best, cu[live], live)
        np.minimum.at(best, cv[live], live)
        roots = np.flatnonzero(best < m)
        assert np.array_equal(comp[roots], roots)
        b = best[roots]
        a, z = comp[eu[b]], comp[ev[b]]
        other = np.where(a == roots, z, a)
        hooks = ~((best[other] == b) & (roots < other))
        dst = comp.copy()
        dst[roots[hooks]] = other[hooks]
        chosen[b[hooks]] = True
        x, depth = np.arange(n), 0                           # compress fully, counting the hops
        while True:
            y = dst[x]
            if np.array_equal(y, x):
                break
            x, depth = y, depth + 1
        comp = x
        depths.append(depth)
    return np.sort(order[chosen]), len(depths), depths


# ---- builders --------------------------------------------------------------------------------------------------------
def two_chains(n):
    """(e int64 [m, 2], w float32 [m], tree): chain A on vertices 0 .. h-1 and chain B on h .. n-1, h = n // 2.  In
    this order: the chain edges (k, k+1) at (k - first + 1) * 2^-20, strictly increasing along each chain; the cross
    edges (c, c+h), c < min(h, n-h), at 4 + c * 2^-18; the chords (k, k+2) inside each chain at 2 + (k - first) * 2^-18.
    Every vertex's least edge goes to its predecessor (the first vertex's to its successor), so round one hooks each
    chain into one tree as deep as the chain is long, less one; round two joins the two by (0, h) only if every vertex
    was compressed to its root.  The forest is the n - 2 chain edges and that cross edge: tree = arange(n - 1)."""
    assert 4 <= n <= 1 << 20
    h = n // 2
    parts_e, parts_w = [], []
    for first, last in ((0, h - 1), (h, n - 1)):             # chain edges
        k = np.arange(first, last)
        parts_e.append(np.stack([k, k + 1], axis=1))
        parts_w.append((k - first + 1) * 2.0 ** -20)
    c = np.arange(min(h, n - h))                             # cross edges
    parts_e.append(np.stack([c, c + h], axis=1))
    parts_w.append(4.0 + c * 2.0 ** -18)
    for first, last in ((0, h - 1), (h, n - 1)):             # chords
        k = np.arange(first, last - 1)
        parts_e.append(np.stack([k, k + 2], axis=1))
        parts_w.append(2.0 + (k - first) * 2.0 ** -18)
    e = np.concatenate(parts_e).astype(np.int64)
    w64 = np.concatenate(parts_w)
    w = w64.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), w64)         # the round trip: every weight is a float32
    return e, w, np.arange(n - 1, dtype=np.int64)


def ruler(n):
    """(e, w, tree): the path (k, k+1) at weight ctz(k + 1), then the chords (k, k+3) at 64 + k, which are never
    chosen.  The two path edges at a vertex always differ in weight (one of k, k + 1 is odd), so no choice is tied; at
    n = 2^k round r merges blocks of 2^(r-1) pairwise and the forest needs exactly k rounds.  tree = arange(n - 1)."""
    assert 2 <= n <= 1 << 20
    k = np.arange(n - 1, dtype=np.int64)
    ctz = np.log2((k + 1) & -(k + 1)).astype(np.int64)
    assert np.array_equal(1 << ctz, (k + 1) & -(k + 1))
    c = np.arange(max(n - 3, 0), dtype=np.int64)
    e = np.concatenate([np.stack([k, k + 1], axis=1), np.stack([c, c + 3], axis=1)])
    w = np.concatenate([ctz, 64 + c]).astype(np.float32)
    return e, w, np.arange(n - 1, dtype=np.int64)


def equal_weights(n, seed):
    """(e, w): about 2.5 n random pairs in either orientation with about 10 % parallel copies, the edges (0, n-1),
    (1, n-1), (n-2, n-1) and (n/2, n/2 + 1) where they are edges of n vertices, a few vertices left isolated (n >= 16),
    every weight 0.5: the forest is decided by (min, max, index) alone."""
    assert n >= 2
    rng = np.random.default_rng(seed)
    fixed = np.array([(0, n - 1), (1, n - 1), (n - 2, n - 1), (n // 2, n // 2 + 1)], dtype=np.int64)
    fixed = fixed[(fixed[:, 0] != fixed[:, 1]) & (fixed.max(axis=1) < n)]
    live = np.arange(n)
    if n >= 16:
        inner = np.setdiff1d(live, fixed.ravel())
        live = np.setdiff1d(live, rng.choice(inner, 3, replace=False))
    count = max(int(2.5 * n), 1)
    a = live[rng.integers(0, live.size, count)]
    b = live[(np.searchsorted(live, a) + rng.integers(1, live.size, count)) % live.size]
    e = np.stack([a, b], axis=1)
    e = np.concatenate([e, fixed, e[rng.random(count) < 0.1], fixed[:, ::-1]])
    e = e[rng.permutation(len(e))]
    assert (e[:, 0] != e[:, 1]).all() and e.min() >= 0 and e.max() < n
    return e.astype(np.int64), np.full(len(e), 0.5, dtype=np.float32)


def weight_levels(rng):
    """float32 [26]: both zeros, the least subnormal, the least normal, 1 and its two neighbours and the largest finite
    value, each of either sign, and a dozen random values of either sign over 2^+-60."""
    one = np.float32(1.0)
    pos = np.array([0.0, 1.4e-45, 1.17549435e-38, 1.0, np.nextafter(one, np.float32(2.0)),
                    np.nextafter(one, np.float32(0.0)), 3.4028235e38], dtype=np.float32)
    more = np.ldexp(rng.uniform(1.0, 2.0, 12), rng.integers(-60, 61, 12)) * np.where(rng.random(12) < 0.5, -1.0, 1.0)
    vals = np.concatenate([pos, -pos, more.astype(np.float32)]).astype(np.float32)
    assert np.isfinite(vals).all() and np.signbit(vals[7]) and vals[7] == 0.0
    return vals


def weight_range(n, seed):
    """(e, w): `multigraph` with weights drawn from weight_levels: the whole finite float32 range, ties at each.  Half
    of the vertices it leaves isolated then get a block of their own, about three random pairs a vertex in either
    orientation, every weight +0.0 or -0.0: inside the block the forest is decided by (min, max, index) across the two
    signs, which the graph's lighter (negative) edges would otherwise have settled before a zero is looked at.  The
    edges are shuffled together."""
    rng = np.random.default_rng(seed)
    vals = weight_levels(rng)
    e, w = multigraph(rng, n, max(n // 400, 3), 10 * n, len(vals), vals=vals)
    block = np.setdiff1d(np.arange(n), e.ravel())[::2]
    k = block.size
    assert k >= 16
    a = rng.integers(0, k, 3 * k)
    b = (a + rng.integers(1, k, 3 * k)) % k
    zero = np.where(rng.random(3 * k) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    e = np.concatenate([e, np.stack([block[a], block[b]], axis=1)])
    w = np.concatenate([w, zero])
    p = rng.permutation(len(e))
    return e[p].astype(np.int64), w[p]


def known_forest(n, comps, isolated, m, seed):
    """(e, w, tree, labels) with its answer by construction.  The vertices are randomly permuted; the last `isolated`
    get no edge, the rest are cut into `comps` runs.  Inside a run every position after the first picks a uniformly
    random earlier position as its parent (a random recursive tree); these forest edges weigh one of 64 levels in
    [0, 1).  The other m - (forest edges) entries are chords between two different positions of one run, in [2, 3).
    Edges are shuffled and half are flipped.  Every forest edge is lighter than every chord and the forest spans every
    run, so under any tie order the minimum spanning forest is the forest edges: tree holds their indices.  labels are
    the ranks of each component's smallest vertex."""
    rng = np.random.default_rng(seed)
    na = n - isolated
    assert comps >= 1 and na >= 4 * comps
    perm = rng.permutation(n)
    cuts = 2 * np.sort(rng.choice(np.arange(1, na // 2), comps - 1, replace=False))     # every run holds 2 or more
    starts = np.concatenate([[0], cuts]).astype(np.int64)
    lens = np.diff(np.concatenate([starts, [na]]))
    pos = np.arange(na, dtype=np.int64)
    run = np.searchsorted(starts, pos, side="right") - 1
    off = pos - starts[run]
    child = pos[off > 0]
    parent = starts[run[child]] + (rng.random(child.size) * off[child]).astype(np.int64)
    assert (parent < child).all() and (parent >= starts[run[child]]).all()
    nf = child.size
    assert nf == na - comps and m >= nf
    ca = rng.integers(0, na, m - nf)                                                    # chords
    la = lens[run[ca]]
    cb = starts[run[ca]] + (off[ca] + rng.integers(1, la)) % la
    assert (ca != cb).all() and np.array_equal(run[ca], run[cb])
    e = np.stack([np.concatenate([parent, ca]), np.concatenate([child, cb])], axis=1)
    e = perm[e].astype(np.int64)
    w = np.concatenate([rng.integers(0, 64, nf) / 64.0, 2.0 + rng.integers(0, 1 << 20, m - nf) * 2.0 ** -20])
    p = rng.permutation(m)
    e, w = e[p], w[p].astype(np.float32)
    flip = rng.random(m) < 0.5
    e[flip] = e[flip][:, ::-1]
    tree = np.flatnonzero(p < nf)
    comp_of = np.empty(n, dtype=np.int64)                                               # by vertex
    comp_of[perm[:na]] = run
    comp_of[perm[na:]] = comps + np.arange(isolated)
    least = np.full(comps + isolated, n, dtype=np.int64)
    np.minimum.at(least, comp_of, np.arange(n))
    labels = np.searchsorted(np.sort(least), least[comp_of]).astype(np.int32)
    return e, w, tree, labels


def euclid_rows(n, seed):
    """float32 [n (n - 1) / 2, 2] distance rows over the float range: ldexp(u, e), u uniform in [1, 2), e a uniform
    integer in [-80, 63]; about 2 % of rows with a zero (of either sign) in one or both columns; eight rows subnormal
    in one or both columns.  Where e is 63 or so x0^2 + x1^2 overflows to inf in float32; below -63 or so the squares
    are subnormal or zero."""
    rng = np.random.default_rng(seed)
    rows = n * (n - 1) // 2
    x = np.ldexp(rng.uniform(1.0, 2.0, (rows, 2)), rng.integers(-80, 64, (rows, 2))).astype(np.float32)
    z = rng.random(rows) < 0.02
    which = rng.integers(0, 3, rows)                         # column 0, column 1, both
    zero = np.where(rng.random(rows) < 0.5, np.float32(-0.0), np.float32(0.0))
    x[z & (which != 1), 0] = zero[z & (which != 1)]
    x[z & (which != 0), 1] = zero[z & (which != 0)]
    sub = rng.choice(rows, 8, replace=False)
    x[sub[:6], 0] = np.ldexp(rng.uniform(1.0, 2.0, 6), rng.integers(-149, -127, 6)).astype(np.float32)
    x[sub[4:], 1] = np.ldexp(rng.uniform(1.0, 2.0, 4), rng.integers(-149, -127, 4)).astype(np.float32)
    return x


def euclid_expected(x):
    """float32 [rows]: sqrt(x0*x0 + x1*x1) with every operation rounded to float32.  The root is taken in double and
    rounded once more, which is the correctly rounded float32 root because 53 >= 2 * 24 + 2."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        s = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]
    assert s.dtype == np.float32
    return np.sqrt(s.astype(np.float64)).astype(np.float32)


def all_pairs(n):
    """int64 [n (n - 1) / 2, 2]: every (i, j), i < j, in the condensed matrix's row order."""
    i, j = np.triu_indices(n, 1)
    return np.stack([i, j], axis=1).astype(np.int64)
