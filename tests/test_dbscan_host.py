"""CPU tests of the DBSCAN (HDBSCAN) model: the numpy restatement of include/ppk.h's DBSCAN section lives here
(the GPU tests import it), and poppunk_amd/dbscan.py's hierarchy, the PopPUNK glue and the npz format are checked
against it, against sklearn (committed goldens, tests/golden/dbscan_*.npz) and on hand-made cases."""
import glob
import heapq
import os

import numpy as np
import pytest

from poppunk_amd import dbscan

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan_*.npz")))
DBL_MAX = np.finfo(np.float64).max


# ---- the restatement ---------------------------------------------------------------------------------------------
def ref_d2(P):
    """float64 [n, n]: d2(a, b) = (double)(ax - bx)^2 + (double)(ay - by)^2."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    dx = P[:, None, 0] - P[None, :, 0]
    dy = P[:, None, 1] - P[None, :, 1]
    return dx * dx + dy * dy


def ref_core2(P, m):
    d2 = ref_d2(P)
    np.fill_diagonal(d2, np.inf)
    return np.partition(d2, m - 1, axis=1)[:, m - 1]


def ref_mst_kruskal(P, core2):
    """Kruskal over every pair sorted by (mr2, lo, hi): the definition, for small n."""
    n = len(P)
    mr2 = np.maximum(np.maximum(core2[:, None], core2[None, :]), ref_d2(P))
    lo, hi = np.triu_indices(n, 1)
    w = mr2[lo, hi]
    order = np.lexsort((hi, lo, w))
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    out = []
    for e in order:
        ra, rb = find(lo[e]), find(hi[e])
        if ra != rb:
            par[ra] = rb
            out.append((lo[e], hi[e], w[e]))
            if len(out) == n - 1:
                break
    return (np.array([e[0] for e in out], dtype=np.int32), np.array([e[1] for e in out], dtype=np.int32),
            np.array([e[2] for e in out], dtype=np.float64))


def ref_mst(P, core2):
    """The same tree by Prim under the same total order (the minimum spanning tree is unique under a total order),
    O(n^2) in numpy, sorted by (mr2, lo, hi)."""
    P64 = np.asarray(P, dtype=np.float32).astype(np.float64)
    n = len(P64)
    idx = np.arange(n)

    def keys_from(u):
        dx, dy = P64[u, 0] - P64[:, 0], P64[u, 1] - P64[:, 1]
        return np.maximum(np.maximum(core2[u], core2), dx * dx + dy * dy), np.minimum(u, idx), np.maximum(u, idx)
    in_tree = np.zeros(n, dtype=bool)
    in_tree[0] = True
    bw, blo, bhi = keys_from(0)
    ew, elo, ehi = np.empty(n - 1), np.empty(n - 1, dtype=np.int64), np.empty(n - 1, dtype=np.int64)
    for k in range(n - 1):
        w = np.where(in_tree, np.inf, bw)
        cand = np.flatnonzero(w == w.min())
        v = cand[np.lexsort((bhi[cand], blo[cand]))[0]]
        ew[k], elo[k], ehi[k] = bw[v], blo[v], bhi[v]
        in_tree[v] = True
        nw, nlo, nhi = keys_from(v)
        better = ~in_tree & ((nw < bw) | ((nw == bw) & ((nlo < blo) | ((nlo == blo) & (nhi < bhi)))))
        bw, blo, bhi = np.where(better, nw, bw), np.where(better, nlo, blo), np.where(better, nhi, bhi)
    order = np.lexsort((ehi, elo, ew))
    return elo[order].astype(np.int32), ehi[order].astype(np.int32), ew[order]


def ref_hierarchy(a, b, mr2, n, c):
    """Single linkage with explicit member lists, the condensed tree by walking down from each cluster's top node,
    stabilities and excess of mass by recursion.  Returns a dict of the arrays a fit keeps, and the labels."""
    members, owner, kids = {i: [i] for i in range(n)}, list(range(n)), {}
    for k in range(n - 1):
        L, R = owner[a[k]], owner[b[k]]
        assert L != R
        node = n + k
        members[node] = members[L] + members[R]
        d = float(np.sqrt(mr2[k]))
        kids[node] = (L, R, (1.0 / d) if d > 0.0 else np.inf)
        for p in members[node]:
            owner[p] = node
    pt_cluster, pt_lambda = np.full(n, -1, dtype=np.int32), np.zeros(n)
    cl_parent, cl_birth, cl_size = [-1], [0.0], [n]

    def descend(node, cl):
        """Follow the cluster down to the node where it truly splits (returned) or dissolves (None)."""
        while node >= n:
            L, R, lam = kids[node]
            nl, nr = len(members[L]), len(members[R])
            if nl >= c and nr >= c:
                return node
            for side, cnt in ((L, nl), (R, nr)):
                if cnt < c:
                    for p in members[side]:
                        pt_cluster[p], pt_lambda[p] = cl, lam
            if nl < c and nr < c:
                return None
            node = R if nl < c else L
        return None

    heap = []
    s = descend(2 * n - 2, 0)
    if s is not None:
        heap.append((-s, 0))
    while heap:
        neg, cl = heapq.heappop(heap)       # true splits in decreasing node order
        L, R, lam = kids[-neg]
        for child in (L, R):
            new = len(cl_parent)
            cl_parent.append(cl)
            cl_birth.append(lam)
            cl_size.append(len(members[child]))
            s = descend(child, new)
            if s is not None:
                heapq.heappush(heap, (-s, new))
    n_cl = len(cl_parent)
    children = [[k for k in range(n_cl) if cl_parent[k] == p] for p in range(n_cl)]
    with np.errstate(invalid="ignore"):
        stab = [float(np.sum(pt_lambda[pt_cluster == k] - cl_birth[k])
                      + sum((cl_birth[ch] - cl_birth[k]) * cl_size[ch] for ch in children[k])) for k in range(n_cl)]

    def best(k):
        got = [best(ch) for ch in children[k]]
        sub = sum(g[0] for g in got) if got else 0.0
        if k != 0 and not sub > stab[k]:
            return stab[k], [k]
        return sub, [x for g in got for x in g[1]]
    selected = best(0)[1]
    anc = [-1] * n_cl
    for k in range(1, n_cl):
        anc[k] = k if k in selected else anc[cl_parent[k]]
    pt_sel = np.array([anc[k] for k in pt_cluster])
    firsts = sorted((int(np.flatnonzero(pt_sel == k)[0]), k) for k in selected if np.any(pt_sel == k))
    number = {k: i for i, (_, k) in enumerate(firsts)}
    cl_label = np.array([number.get(anc[k], -1) for k in range(n_cl)], dtype=np.int32)
    return dict(pt_cluster=pt_cluster, pt_lambda=pt_lambda, cl_parent=np.array(cl_parent, dtype=np.int32),
                cl_birth=np.array(cl_birth), cl_label=cl_label), cl_label[pt_cluster]


def tie_set(a, b, mr2, n, c):
    """The points whose label may depend on the order of equal-weight edges: walk the sorted tree in runs of equal
    mr2; inside a run group the edges by connectivity over the components as they stood before the run; a group that
    joins >= 3 components whose sizes, the largest left out, sum to >= c is order-dependent, and every point of its
    components smaller than c is tie-affected."""
    par, size = list(range(n)), [1] * n
    members = {i: [i] for i in range(n)}

    def find(x):
        while par[x] != x:
            x = par[x]
        return x
    marked, i = set(), 0
    while i < n - 1:
        j = i
        while j < n - 1 and mr2[j] == mr2[i]:
            j += 1
        if j - i >= 2:
            ed = [(find(a[e]), find(b[e])) for e in range(i, j)]
            g = {}

            def f2(x):
                while g.setdefault(x, x) != x:
                    x = g[x]
                return x
            for x, y in ed:
                g[f2(x)] = f2(y)
            grp = {}
            for x, y in ed:
                grp.setdefault(f2(x), set()).update((x, y))
            for comps in grp.values():
                s = [size[r] for r in comps]
                if len(comps) >= 3 and sum(s) - max(s) >= c:
                    for r in comps:
                        if size[r] < c:
                            marked.update(members[r])
        for e in range(i, j):
            x, y = find(a[e]), find(b[e])
            if size[x] < size[y]:
                x, y = y, x
            par[y] = x
            size[x] += size[y]
            members[x] += members.pop(y)
        i = j
    return marked


def same_partition(x, y):
    """Noise sets identical and a bijection between the cluster ids."""
    x, y = np.asarray(x), np.asarray(y)
    if not np.array_equal(x == -1, y == -1):
        return False
    pairs = set(zip(x.tolist(), y.tolist()))
    return len(pairs) == len(set(x.tolist())) == len(set(y.tolist()))


def ref_fit(P, m, c):
    """(core2, (a, b, mr2), Tree) of the restated MST through poppunk_amd.dbscan's hierarchy."""
    core2 = ref_core2(P, m)
    a, b, mr2 = ref_mst(P, core2)
    return core2, (a, b, mr2), dbscan.fit_tree(a, b, mr2, len(P), c)


def scale_rows(X, scale):
    """X / scale in the dtype numpy promotes to, as float64 for the distance arithmetic."""
    X, scale = np.asarray(X, dtype=np.float32), np.asarray(scale)
    return (X / scale).astype(np.float64) if scale.dtype == np.float32 else X.astype(np.float64) / scale


def _walk(t, lq, tree):
    cl = int(tree.pt_cluster[t])
    if tree.pt_lambda[t] > lq:
        while cl != 0 and tree.cl_birth[cl] >= lq:
            cl = int(tree.cl_parent[cl])
    return int(tree.cl_label[cl])


def ref_assign_row(q, P, core2, m, tree):
    """One scaled row (float64 [2]) through the five steps, by sorting."""
    P64 = np.asarray(P, dtype=np.float32).astype(np.float64)
    n = len(P64)
    dx, dy = q[0] - P64[:, 0], q[1] - P64[:, 1]
    d2 = dx * dx + dy * dy
    order = np.lexsort((np.arange(n), d2))
    N = order[:min(2 * m, n)]
    r2 = d2[order[min(m, n - 1)]]
    w = np.maximum(np.maximum(core2[N], r2), d2[N])
    j = int(np.argmin(w))                                  # the first of N, in its order, at the minimum
    lq = 1.0 / np.sqrt(w[j]) if w[j] > 0.0 else DBL_MAX
    return _walk(int(N[j]), lq, tree)


def ref_assign(Q, P, core2, m, tree, block=2048):
    """The same for float64 [k, 2] scaled rows without a sort per row (selection by partition, ties by cumulative
    count), a block of rows at a time.  test_assignment_block_form_equals_row_form ties it to ref_assign_row."""
    P64 = np.asarray(P, dtype=np.float32).astype(np.float64)
    n = len(P64)
    kk, rr = min(2 * m, n) - 1, min(m, n - 1)
    out = np.empty(len(Q), dtype=np.int32)
    pt_cluster, pt_lambda = np.asarray(tree.pt_cluster), np.asarray(tree.pt_lambda)
    cl_birth, cl_parent, cl_label = np.asarray(tree.cl_birth), np.asarray(tree.cl_parent), np.asarray(tree.cl_label)
    for s in range(0, len(Q), block):
        q = np.asarray(Q[s:s + block], dtype=np.float64)
        dx, dy = q[:, 0:1] - P64[None, :, 0], q[:, 1:2] - P64[None, :, 1]
        d2 = dx * dx + dy * dy
        part = np.partition(d2, sorted({kk, rr}), axis=1)
        vk, r2 = part[:, kk:kk + 1], part[:, rr:rr + 1]
        below, at = d2 < vk, d2 == vk
        quota = kk + 1 - below.sum(axis=1, keepdims=True)
        inN = below | (at & (np.cumsum(at, axis=1) <= quota))
        w = np.where(inN, np.maximum(np.maximum(core2[None, :], r2), d2), np.inf)
        wmin = w.min(axis=1, keepdims=True)
        dc = np.where(w == wmin, d2, np.inf)
        t = np.argmax(dc == dc.min(axis=1, keepdims=True), axis=1)
        wmin = wmin[:, 0]
        with np.errstate(divide="ignore"):
            lq = np.where(wmin > 0.0, 1.0 / np.sqrt(wmin), DBL_MAX)
        cl = pt_cluster[t].astype(np.int64)
        climb = pt_lambda[t] > lq
        while True:
            go = climb & (cl != 0) & (cl_birth[cl] >= lq)
            if not go.any():
                break
            cl = np.where(go, cl_parent[cl], cl)
        out[s:s + block] = cl_label[cl]
    return out


def ref_model_fit(sub, max_num_clusters, min_cluster_prop):
    """DBSCANFit.fit's loop (PopPUNK/models.py:515-600) on a scaled float32 subsample, every step restated here.
    Returns the state of the accepted fit, or raises RuntimeError where the reference exits."""
    n = len(sub)
    m, c = min(max(int(min_cluster_prop * n), 10), 1023), max(int(0.01 * n), 10)
    indistinct, out = True, None
    while indistinct and c >= m and m >= 10:
        core2, _, tree = ref_fit(sub, m, c)
        k = tree.n_clusters
        if 1 < k <= max_num_clusters:
            s64 = sub.astype(np.float64)
            means = np.stack([s64[tree.labels == i].mean(axis=0) for i in range(k)])
            mins = np.stack([s64[tree.labels == i].min(axis=0) for i in range(k)])
            maxs = np.stack([s64[tree.labels == i].max(axis=0) for i in range(k)])
            y = ref_assign(s64, sub, core2, m, tree)
            present = [i for i in range(k) if np.any(y == i)]
            within = min(present, key=lambda i: (float(np.hypot(*means[i])), i))
            others = [i for i in present if i != within]
            if others:
                between = max(others, key=lambda i: (int((y == i).sum()), -i))
                indistinct = not (mins[between, 0] > maxs[within, 0] or mins[between, 1] > maxs[within, 1])
                out = dict(core2=core2, tree=tree, m=m, c=c, within=within, between=between, means=means, mins=mins,
                           maxs=maxs, y=y)
        if c < m / 2:
            m = m // 10
        c = int(c / 2)
    if indistinct:
        raise RuntimeError("Failed to find distinct clusters in this dataset")
    return out


def blobs(n, seed, dup=0):
    """Small planted input: two blobs and uniform noise, float32 in [0, 1], `dup` points repeated."""
    rng = np.random.default_rng(seed)
    k = n // 3
    X = np.vstack([rng.normal([0.1, 0.1], 0.03, (k, 2)), rng.normal([0.7, 0.6], 0.06, (n - k - n // 10, 2)),
                   rng.uniform(0, 1, (n // 10, 2))])
    X = np.abs(X).astype(np.float32)[rng.permutation(n)]
    if dup:
        X[rng.choice(n, dup, replace=False)] = X[rng.choice(n, dup)]
    return X / X.max(axis=0)


# ---- 1. restatement vs poppunk_amd.dbscan ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,c,seed,dup", [(60, 3, 5, 0, 0), (150, 5, 8, 1, 0), (150, 10, 10, 2, 40), (300, 10, 12, 3, 0),
                                            (40, 39, 4, 4, 0)])
def test_hierarchy_equals_the_restatement(n, m, c, seed, dup):
    P = blobs(n, seed, dup)
    core2 = ref_core2(P, m)
    a, b, mr2 = ref_mst_kruskal(P, core2)
    a2, b2, mr22 = ref_mst(P, core2)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(mr2.view(np.uint64), mr22.view(np.uint64))
    want, want_labels = ref_hierarchy(a, b, mr2, n, c)
    got = dbscan.fit_tree(a, b, mr2, n, c)
    assert np.array_equal(got.labels, want_labels)
    for k, v in want.items():
        assert np.array_equal(np.asarray(getattr(got, k)), v), k


def test_single_linkage_refuses_a_cycle():
    with pytest.raises(ValueError):
        dbscan.single_linkage([0, 0, 1], [1, 1, 2], [1.0, 1.0, 1.0], 4)


def test_no_cluster_means_all_noise():
    P = np.random.default_rng(0).uniform(0, 1, (30, 2)).astype(np.float32)
    _, _, tree = ref_fit(P, 3, 40)
    assert tree.n_clusters == 0 and np.all(tree.labels == -1) and tree.cl_parent.tolist() == [-1]


# ---- 2. against sklearn (committed labels) -------------------------------------------------------------------------------
def load_golden(path):
    with np.load(path, allow_pickle=False) as z:
        return z["points"], int(z["m"]), int(z["c"]), z["sklearn_labels"], bool(z["equal_everywhere"])


def check_against_golden(labels, mst, points, c, sk, whole, what):
    n = len(points)
    T = tie_set(*mst, n, c)
    keep = np.ones(n, dtype=bool)
    keep[list(T)] = False
    print("%s: n %d, clusters %d, noise %d, |T| %d, equal off T %s, equal everywhere %s"
          % (what, n, len(set(sk.tolist())) - (1 if -1 in sk else 0), int((sk == -1).sum()), len(T),
             same_partition(labels[keep], sk[keep]), same_partition(labels, sk)))
    assert len(T) <= 0.05 * n
    assert same_partition(labels[keep], sk[keep])
    if whole:
        assert same_partition(labels, sk)


def test_goldens_are_committed():
    cases = [load_golden(p) for p in GOLDEN]
    assert len(cases) >= 6
    assert min(len(c[0]) for c in cases) <= 500 and max(len(c[0]) for c in cases) >= 4000
    assert sum(c[4] for c in cases) >= 2


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_labels_equal_sklearn_off_the_tie_affected_points(path):
    points, m, c, sk, whole = load_golden(path)
    assert points.dtype == np.float32
    _, mst, tree = ref_fit(points, m, c)
    check_against_golden(tree.labels, mst, points, c, sk, whole, os.path.basename(path))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_goldens_still_are_what_sklearn_gives(path):
    cluster = pytest.importorskip("sklearn.cluster")
    points, m, c, sk, _ = load_golden(path)
    now = cluster.HDBSCAN(min_samples=m + 1, min_cluster_size=c, algorithm="kd_tree").fit(points.astype(np.float64)).labels_
    assert same_partition(now, sk)


# ---- 3. PopPUNK's glue ---------------------------------------------------------------------------------------------------
def test_parameter_rules():
    assert dbscan.min_samples_for(100000, 0.0001) == 10
    assert dbscan.min_samples_for(100000, 0.005) == 500
    assert dbscan.min_samples_for(100000, 0.5) == 1023
    assert dbscan.min_cluster_size_for(500) == 10 and dbscan.min_cluster_size_for(100000) == 1000
    # the halving step: min_samples drops tenfold only once min_cluster_size is under half of it
    assert dbscan.next_parameters(100, 1000) == (100, 500)
    assert dbscan.next_parameters(100, 49) == (10, 24)
    assert dbscan.next_parameters(100, 50) == (100, 25)
    assert dbscan.loop_continues(True, 10, 10) and not dbscan.loop_continues(False, 10, 10)
    assert not dbscan.loop_continues(True, 11, 10) and not dbscan.loop_continues(True, 9, 100)
    assert dbscan.acceptable(2, 2) and not dbscan.acceptable(1, 5) and not dbscan.acceptable(6, 5)


def test_within_and_between_labels():
    means = np.array([[0.5, 0.5], [0.05, 0.04], [0.01, 0.01], [0.9, 0.9]])
    y = np.array([0, 0, 0, 1, 1, -1, 3, 3, 3, 3, -1, -1, -1, -1, -1])
    assert dbscan.findWithinLabel(means, y) == 1          # label 2 is closer but nobody carries it
    assert dbscan.findWithinLabel(means, y, rank=1) == 0
    assert dbscan.findBetweenLabel(y, 1) == 3             # the most frequent, noise and within left out
    assert dbscan.findBetweenLabel(np.array([1, 1, 0, 2, 2, 0]), 1) == 0   # equally frequent: the lower label
    with pytest.raises(ValueError):
        dbscan.findBetweenLabel(np.array([1, 1, -1]), 1)


def test_indistinct_clusters():
    mins = np.array([[0.0, 0.0], [0.3, 0.1]])
    maxs = np.array([[0.2, 0.4], [0.9, 0.9]])
    assert not dbscan.evaluate_dbscan_clusters(mins, maxs, 0, 1)          # core ranges apart
    assert dbscan.evaluate_dbscan_clusters(np.array([[0.0, 0.0], [0.1, 0.1]]), maxs, 0, 1)   # both overlap
    assert not dbscan.evaluate_dbscan_clusters(np.array([[0.0, 0.0], [0.1, 0.5]]), maxs, 0, 1)   # accessory apart


def test_fit_loop_on_a_planted_mixture_and_on_noise():
    points = load_golden([p for p in GOLDEN if p.endswith("dbscan_1500_1.npz")][0])[0]
    fit = ref_model_fit(points, 5, 0.01)
    assert (fit["m"], fit["c"]) == (15, 15)                      # accepted at the first pair of parameters
    assert fit["within"] == int(np.argmin(np.hypot(fit["means"][:, 0], fit["means"][:, 1])))
    assert fit["within"] == dbscan.findWithinLabel(fit["means"], fit["y"])
    assert fit["between"] == dbscan.findBetweenLabel(fit["y"], fit["within"])
    assert np.bincount(fit["y"][fit["y"] >= 0]).argmax() == fit["between"]   # the large between-strain blob
    with pytest.raises(RuntimeError, match="distinct clusters"):
        ref_model_fit(points, 1, 0.01)                            # no fit may have more than one cluster: never accepted
    uniform = np.random.default_rng(5).uniform(0, 1, (400, 2)).astype(np.float32)
    with pytest.raises(RuntimeError, match="distinct clusters"):
        ref_model_fit(uniform, 2, 0.01)


# ---- 4. the assignment restatement -------------------------------------------------------------------------------------------
def planted_rows(P, rng):
    """float32 rows (already scaled): on training points, midway between two, outside the cloud, and random."""
    P = np.asarray(P, dtype=np.float32)
    on = P[rng.choice(len(P), 8)]
    # exactly the same distance from two training points: (x, y) and (x + 2h, y), the row at (x + h, y)
    mid = np.array([[0.5, 0.25]], dtype=np.float32)
    outside = np.array([[3.0, 3.0], [-1.0, 0.5], [0.0, 40.0]], dtype=np.float32)
    return np.vstack([on, mid, outside, rng.uniform(0, 1, (40, 2)).astype(np.float32)])


def with_index_tie(P):
    """Two training points at the same distance from the row (0.5, 0.25): 0.4375 and 0.5625 are 0.5 -+ 2^-4."""
    P = np.array(P, dtype=np.float32)
    P[3] = (0.4375, 0.25)
    P[11] = (0.5625, 0.25)
    return P


@pytest.mark.parametrize("n,m,c,seed", [(200, 10, 10, 0), (120, 5, 6, 1), (15, 10, 3, 2)])
def test_assignment_block_form_equals_row_form(n, m, c, seed):
    P = with_index_tie(blobs(n, seed, dup=5))
    core2, _, tree = ref_fit(P, m, c)
    Q = np.vstack([P, planted_rows(P, np.random.default_rng(seed))]).astype(np.float64)
    rows = np.array([ref_assign_row(q, P, core2, m, tree) for q in Q])
    assert np.array_equal(rows, ref_assign(Q, P, core2, m, tree, block=64))


def test_assignment_planted_rows():
    P = with_index_tie(blobs(200, 0))
    m, c = 10, 10
    core2, _, tree = ref_fit(P, m, c)
    assert tree.n_clusters >= 2
    own = ref_assign(P.astype(np.float64), P, core2, m, tree)
    # a training point's own row: every w2 is at least r2 = its own core2, which its own entry (first in the order,
    # d2 = 0) reaches, so t* is the point itself; it left its cluster at an edge no shorter than its core distance,
    # so nothing climbs, and the label is the fitted one -- noise included
    assert np.array_equal(own, tree.labels)
    # w2 = 0: a row on a point repeated more than 2m times
    Pd = P.copy()
    Pd[:25] = Pd[0]
    core2d, _, treed = ref_fit(Pd, m, c)
    assert core2d[0] == 0.0
    assert ref_assign_row(Pd[0].astype(np.float64), Pd, core2d, m, treed) == ref_assign(
        Pd[:1].astype(np.float64), Pd, core2d, m, treed)[0]
    # the index tie: both neighbours at the same d2, the lower index first in the order
    q = np.array([0.5, 0.25])
    d2 = (q[0] - P[:, 0].astype(np.float64)) ** 2 + (q[1] - P[:, 1].astype(np.float64)) ** 2
    assert d2[3] == d2[11]
    # far outside: every w2 is the row's own r2, the first of the order wins, and the walk ends at the root: noise
    assert ref_assign_row(np.array([40.0, 40.0]), P, core2, m, tree) == -1


def test_scale_rows_dtype_rule():
    X = np.array([[0.3, 0.7]], dtype=np.float32)
    s32, s64 = np.array([0.9, 0.8], dtype=np.float32), np.array([0.9, 0.8])
    assert np.array_equal(scale_rows(X, s32), (X / s32).astype(np.float64))
    assert scale_rows(X, s64).dtype == np.float64 and not np.array_equal(scale_rows(X, s64), scale_rows(X, s32))


# ---- 4b. the inputs of tests/test_gpu_dbscan_shapes.py reach what they were built for ---------------------------------------
@pytest.mark.parametrize("n", [16, 34, 514, 4096])
def test_two_chains_hook_into_two_deep_trees(n):
    import dbscan_shapes as S
    P = S.two_chains(n)                                       # (asserts the float32 round trip itself)
    assert P.dtype == np.float32 and P.shape == (n, 2)
    h = n // 2
    assert np.all(P[:h, 1] == 0.0) and np.all(P[h:, 1] == 64.0)
    for chain in (P[:h, 0].astype(np.float64), P[h:, 0].astype(np.float64)):
        gaps = np.diff(chain)
        assert np.all(gaps > 0) and np.all(np.diff(gaps) < 0)
    partner = S.least_partner(P, ref_core2(P, 1))
    assert np.array_equal(partner, S.chain_successors(n))
    # followed from any point, the least edges reach the chain's last pair: one tree per chain, about n / 2 deep
    assert partner[h - 2] == h - 1 and partner[h - 1] == h - 2 and partner[n - 2] == n - 1 and partner[n - 1] == n - 2


def test_lattice_ties():
    import dbscan_shapes as S
    P = S.lattice(33)
    assert P.shape == (1089, 2) and np.array_equal(P[34], np.float32([1 / 32, 1 / 32]))
    core2 = ref_core2(P, 4)
    assert len(np.unique(core2)) == 3                         # corner, side and inner points
    assert len(np.unique(ref_mst(P, core2)[2])) == 3
    # many rows tie exactly at the rank: an inner point has four neighbours at each of its 4th and 8th distances
    d2 = np.sort(ref_d2(P)[33 * 16 + 16])
    assert d2[1] == d2[4] < d2[5] == d2[8] < d2[9]
    P = S.lattice(22)
    core2 = ref_core2(P, 4)
    for x, y in zip(ref_mst(P, core2), ref_mst_kruskal(P, core2)):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y)


def test_wide_range_spans_the_exponent_passes():
    import dbscan_shapes as S
    P = S.wide_range(2049, 0)
    assert P.dtype == np.float32 and np.all(np.isfinite(P)) and np.all(P != 0)
    core2 = ref_core2(P, 7)
    assert np.all(np.isfinite(core2)) and np.all(core2 > 0)
    e = np.frexp(core2)[1]
    assert e.min() <= -100 and e.max() >= 100
    # the six two-bit passes over the exponent field each branch more than one way across the rows
    key = core2.view(np.uint64)
    for shift in range(62, 50, -2):
        assert len(np.unique((key >> np.uint64(shift)) & np.uint64(3))) >= 2, shift


def test_grid_restatement_and_the_row_sets_of_the_tall_grid():
    import dbscan_shapes as S
    P, rows = S.tall_grid_points()
    assert P.shape == (20000, 2) and rows.shape == (4000, 2)
    G = S.grid_of(P)
    assert G.g == 70 and G.count.sum() == 20000 and G.count.shape == (70, 70)
    assert np.array_equal(G.count, np.histogram2d(G.cy, G.cx, bins=[np.arange(71), np.arange(71)])[0])
    A, tall, whole = S.tall_grid_row_sets(G, rows, S.TALL_M)
    assert len(tall) == 761 and len(A) > 0 and len(whole) > 0
    assert set(A.tolist()) <= set(tall.tolist()) and not set(whole.tolist()) & set(tall.tolist())
    print("first 1500 rows at m = %d: %d first squares of more than 64 grid rows, set A %d, whole grid at once %d"
          % (S.TALL_M, len(tall), len(A), len(whole)))
    # a row of set A by hand: its square holds the target, the square one step smaller did not
    gr, gc, is_all, dk2, safe = S.first_square(G, rows[A[0]].astype(np.float64), S.TALL_M)
    assert 64 < gr <= 70 and not is_all and dk2 < 0.9 * safe * safe
    # at a small m no square grows that tall: the largest min_samples is what reaches the branch
    assert len(S.tall_grid_row_sets(G, rows, 25)[1]) == 0
    # with the float64 scale of the GPU test the sets are not empty either
    assert len(S.tall_grid_row_sets(G, rows, S.TALL_M, scale=np.array([1.1, 0.9]))[0]) > 0
    # far rows: three fail their first square and regrow into the whole grid; (0.5, 1e6) certifies in a square that
    # spans every column (only the side below it has cells beyond)
    got = []
    for q in S.FAR_ROWS.astype(np.float64):
        gr, gc, is_all, dk2, safe = S.first_square(G, q, S.TALL_M)
        got.append((bool(safe > 0.0 and dk2 < safe * safe), gc == G.g, S.regrown_square_is_all(G, dk2)))
    assert got == [(False, False, True), (False, False, True), (True, True, True), (False, False, True)]
    assert S.scanned_far_rows(G, S.TALL_M) == [0, 1, 3]
    # the blob of this input lies in the first grid rows of every tall square: the count's first run holds the target
    assert not any(S.rows_past_the_64th_decide(G, rows[i].astype(np.float64), S.TALL_M) for i in A)
    # with the blob against the upper edge every row of set A needs the grid rows past its square's 64th
    P2, rows2 = S.tall_grid_points("top")
    G2 = S.grid_of(P2)
    A2, tall2, whole2 = S.tall_grid_row_sets(G2, rows2, S.TALL_M)
    assert G2.g == 70 and len(A2) > 0 and len(whole2) > 0
    assert all(S.rows_past_the_64th_decide(G2, rows2[i].astype(np.float64), S.TALL_M) for i in A2)
    assert S.scanned_far_rows(G2, S.TALL_M) == [0, 2, 3]
    assert len(S.tall_grid_row_sets(G2, rows2, S.TALL_M, scale=np.array([1.1, 0.9]))[0]) > 0
    print("blob against the upper edge: %d tall first squares, set A %d, whole grid at once %d" % (len(tall2), len(A2), len(whole2)))
    # the whole grid at once when the training set is smaller than the target
    Ps = blobs(100, 0)
    assert S.first_square(S.grid_of(Ps), np.array([0.5, 0.5]), 40)[2]
    # a box without width or height has cells of width 1.0 there
    line = np.stack([np.full(400, 0.5, dtype=np.float32), np.linspace(0, 1, 400, dtype=np.float32)], axis=1)
    Gl = S.grid_of(line)
    assert (Gl.g, Gl.wx) == (10, 1.0) and Gl.wy == pytest.approx(0.1) and np.all(Gl.cx == 0)


@pytest.mark.parametrize("n,n_cl", [(300, 200), (2300, 500)])
def test_assignment_block_form_equals_row_form_on_a_deep_chain(n, n_cl):
    import dbscan_shapes as S
    m = 10
    M = S.synthetic_model(n, n_cl, np.random.default_rng(n))
    assert M.cl_parent[0] == -1 and np.all(M.cl_parent[1:] < np.arange(1, n_cl)) and np.all(M.cl_parent[1:] >= 0)
    assert np.array_equal(M.cl_parent[1:n_cl // 2 + 1], np.arange(n_cl // 2))
    assert np.all(M.core2 > 0) and np.all(M.cl_birth[1:] > 0) and np.all(M.pt_lambda > 0)
    assert set(np.unique(M.cl_label).tolist()) == {-1, 0, 1, 2, 3, 4} and M.n_clusters == 5
    Q = np.vstack([M.points[::5], planted_rows(M.points, np.random.default_rng(1)),
                   np.random.default_rng(2).uniform(-3, 4, (200, 2)).astype(np.float32)]).astype(np.float64)
    rows = np.array([ref_assign_row(q, M.points, M.core2, m, M) for q in Q])
    assert np.array_equal(rows, ref_assign(Q, M.points, M.core2, m, M, block=64))
    assert len(np.unique(rows)) == 6
    assert max(S.walk_depth(q, M, m) for q in Q) >= n_cl // 4


# ---- 5. persistence ----------------------------------------------------------------------------------------------------------
def host_model(P, m, c, within=0, between=1):
    """A DBSCANModel filled from the restatement (no device)."""
    from poppunk_amd.models import DBSCANModel
    core2, _, tree = ref_fit(P, m, c)
    model = DBSCANModel()
    model._set_state(P, core2, tree, m, c)
    k = tree.n_clusters
    model.n_clusters = k
    model.cluster_means = np.stack([P[tree.labels == i].astype(np.float64).mean(axis=0) for i in range(k)])
    model.cluster_mins = np.stack([P[tree.labels == i].astype(np.float64).min(axis=0) for i in range(k)])
    model.cluster_maxs = np.stack([P[tree.labels == i].astype(np.float64).max(axis=0) for i in range(k)])
    model.within_label, model.between_label = within, between
    model.scale = np.array([0.02, 0.4], dtype=np.float32)
    model.fitted = True
    return model


def test_npz_round_trip(tmp_path):
    from poppunk_amd.models import DBSCANModel
    model = host_model(blobs(200, 0), 10, 10)
    path = model.save(str(tmp_path / "db"))
    assert path.endswith("db_fit.npz")
    with np.load(path, allow_pickle=False) as z:
        for k in ("n_clusters", "within", "between", "means", "maxs", "mins", "scale", "assign_points", "use_gpu"):
            assert k in z.files
    back = DBSCANModel.from_npz(path)
    for k in DBSCANModel._STATE:
        a, b = getattr(model, k), getattr(back, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert (back.min_samples, back.min_cluster_size, back.within_label, back.between_label, back.n_clusters) == \
        (model.min_samples, model.min_cluster_size, model.within_label, model.between_label, model.n_clusters)
    assert back.scale.dtype == np.float32 and np.array_equal(back.scale, model.scale) and back.fitted


def test_foreign_fits_are_refused(tmp_path):
    from poppunk_amd.models import BGMMModel, DBSCANModel
    poppunk_dbscan = dict(n_clusters=2, within=0, between=1, means=np.zeros((2, 2)), maxs=np.ones((2, 2)),
                          mins=np.zeros((2, 2)), scale=np.ones(2, dtype=np.float32), assign_points=True, use_gpu=False)
    with pytest.raises(ValueError, match="pickled hdbscan.HDBSCAN"):
        DBSCANModel.from_npz(poppunk_dbscan)
    bgmm = dict(weights=np.ones(2) / 2, means=np.zeros((2, 2)), covariances=np.stack([np.eye(2)] * 2),
                scale=np.ones(2, dtype=np.float32), within=0, between=1)
    with pytest.raises(ValueError, match="BGMM fit"):
        DBSCANModel.from_npz(bgmm)
    with pytest.raises(ValueError, match="refine"):
        DBSCANModel.from_npz(dict(intercept=0.0))
    # a fit this model wrote is still a DBSCAN fit to BGMMModel
    path = host_model(blobs(200, 0), 10, 10).save(str(tmp_path / "db"))
    with pytest.raises(ValueError, match="DBSCAN fit"):
        BGMMModel.from_npz(path)


def test_unfitted_model_is_an_error():
    from poppunk_amd.models import DBSCANModel
    with pytest.raises(RuntimeError):
        DBSCANModel().assign(np.zeros((1, 2), dtype=np.float32))
    with pytest.raises(RuntimeError):
        DBSCANModel().save("nowhere")
