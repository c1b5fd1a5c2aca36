"""Plain, exact references and designed graphs for the network kernels (ppk_network.hip).

References: sweep_counts (the four integers of every G_t, from their definitions), labels (scipy), brandes_exact
(Brandes in integers and fractions: no rounding of its own), the closed forms, and plan (bt_plan_kernel's arithmetic,
restated, to prove on the CPU that a designed graph reaches the branch it was designed for).

Generators: every one is seeded, gives each unordered pair once, flips the orientation of edges at random and permutes
them.  Ids are shuffled except where the id order is the point of the graph (hub_graph, triangle_orderings).

No device, no poppunk_amd import: tests/test_network_shapes_host.py checks this module on the CPU and
tests/test_gpu_network_shapes.py uses it."""
import math
from collections import deque
from fractions import Fraction

import numpy as np

BT_ITEMS = 1024            # kBtItems: the work items per graph bt_plan_kernel aims at
BT_SMALL_CAP = 256         # kBtSmallCap
BT_LDS_DEFAULT = 4549      # (160 KiB - 64 - 8) / 36: what bt_lds_max = 0 means where the large LDS launch is granted


# ---- references ------------------------------------------------------------------------------------------------------
def sweep_counts(i, j, o, n, n_off):
    """int64 [n_off][4] = edges, components, triangles, connected triples of every G_t (the edges of offset <= t over
    vertices 0 .. n-1).  Every quantity is attributed to the offset at which it appears and prefix-summed."""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    o = np.asarray(o, dtype=np.int64)
    inc = np.zeros((n_off, 4), dtype=np.int64)
    inc[:, 0] = np.bincount(o, minlength=n_off)
    # components: union-find, one batch per offset; every successful link removes one component at its offset
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    order = np.argsort(o, kind="stable")
    for a, b, t in zip(i[order].tolist(), j[order].tolist(), o[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            inc[t, 1] -= 1
    # connected triples: a vertex's incident offsets in ascending order; the entry at position k closes k triples, all at
    # its own offset (the larger of the pair's two)
    v = np.concatenate([i, j])
    t = np.concatenate([o, o])
    srt = np.lexsort((t, v))
    v, t = v[srt], t[srt]
    first = np.searchsorted(v, v, side="left")
    np.add.at(inc[:, 3], t, np.arange(v.size, dtype=np.int64) - first)
    # triangles u < v < w from neighbour sets, each at the largest of its three offsets
    off = {}
    up = [set() for _ in range(n)]
    for a, b, x in zip(i.tolist(), j.tolist(), o.tolist()):
        lo, hi = (a, b) if a < b else (b, a)
        off[(lo, hi)] = x
        up[lo].add(hi)
    for u in range(n):
        for w1 in up[u]:
            for w2 in up[u] & up[w1]:
                inc[max(off[(u, w1)], off[(w1, w2)], off[(u, w2)]), 2] += 1
    out = np.cumsum(inc, axis=0)
    out[:, 1] += n
    return out


def brute_counts(i, j, o, n, n_off):
    """the same from a dense adjacency matrix (A @ A), graph by graph: the check of sweep_counts, n of a hundred or so"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    A = np.zeros((n, n))
    out = np.zeros((n_off, 4), dtype=np.int64)
    row = np.array([0, n, 0, 0])
    for t in range(n_off):
        sel = o == t
        if sel.any():
            A[i[sel], j[sel]] = 1
            A[j[sel], i[sel]] = 1
            deg = A.sum(1).astype(np.int64)
            row = np.array([int(A.sum()) // 2, connected_components(csr_matrix(A), directed=False)[0],
                            int(round(((A @ A) * A).sum() / 6)), int((deg * (deg - 1) // 2).sum())])
        out[t] = row
    return out


def labels(i, j, o, n, at):
    """(number of components, label of every vertex) of G_at, numbered as scipy's connected_components numbers them"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    sel = np.asarray(o) <= at
    g = coo_matrix((np.ones(int(sel.sum())), (np.asarray(i)[sel], np.asarray(j)[sel])), shape=(n, n))
    return connected_components(g, directed=False)


def components(edges, n):
    """the components of more than 3 vertices as (sorted member list, number of edges), largest first, then by smallest
    member: the order bt_relabel gives them"""
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        adj[a].append(b)
        adj[b].append(a)
    seen = [False] * n
    out = []
    for v in range(n):
        if seen[v]:
            continue
        seen[v] = True
        members, todo = [v], [v]
        while todo:
            u = todo.pop()
            for w in adj[u]:
                if not seen[w]:
                    seen[w] = True
                    members.append(w)
                    todo.append(w)
        if len(members) > 3:
            out.append((sorted(members), sum(len(adj[u]) for u in members) // 2))
    out.sort(key=lambda c: (-len(c[0]), c[0][0]))
    return out, adj


def brandes_exact(edges, n, fractions=False):
    """Normalised betweenness of every vertex within its component, sum over all sources s of delta_s(v) over
    (n_c - 1)(n_c - 2), 0 in components of <= 3 vertices: sigma in Python ints, delta in Fractions.  Returns (values,
    summary): values float64 [n], each the correctly rounded exact value (the list of Fractions itself with
    fractions=True); summary = [(exact maximum as a Fraction, size)] per component of more than 3 vertices."""
    comps, adj = components(edges, n)
    bc = [Fraction(0)] * n
    summary = []
    for members, _ in comps:
        nc = len(members)
        acc = dict.fromkeys(members, Fraction(0))
        for s in members:
            sigma = {s: 1}
            dist = {s: 0}
            order = []
            q = deque([s])
            while q:
                u = q.popleft()
                order.append(u)
                du = dist[u]
                for w in adj[u]:
                    dw = dist.get(w)
                    if dw is None:
                        dw = dist[w] = du + 1
                        sigma[w] = 0
                        q.append(w)
                    if dw == du + 1:
                        sigma[w] += sigma[u]
            # delta(v) = sigma(v) * sum over the neighbours w one level down of (1 + delta(w)) / sigma(w)
            cof = {}
            for v in reversed(order):
                dv = dist[v] + 1
                tot = Fraction(0)
                for w in adj[v]:
                    if dist[w] == dv:
                        tot += cof[w]
                delta = sigma[v] * tot
                cof[v] = (1 + delta) / sigma[v]
                if v != s:
                    acc[v] += delta
        scale = (nc - 1) * (nc - 2)
        for v in members:
            bc[v] = acc[v] / scale
        summary.append((max(bc[v] for v in members), nc))
    if fractions:
        return bc, summary
    return np.array([float(x) for x in bc], dtype=np.float64), summary


def brandes_float(edges, n, reverse_rows=False):
    """the same in float64, rows read in ascending neighbour order (or descending): what plain double arithmetic gives"""
    comps, adj = components(edges, n)
    adj = [sorted(a, reverse=reverse_rows) for a in adj]
    bc = np.zeros(n)
    for members, _ in comps:
        nc = len(members)
        acc = dict.fromkeys(members, 0.0)
        for s in members:
            sigma = {s: 1.0}
            dist = {s: 0}
            order = []
            q = deque([s])
            while q:
                u = q.popleft()
                order.append(u)
                for w in adj[u]:
                    if w not in dist:
                        dist[w] = dist[u] + 1
                        sigma[w] = 0.0
                        q.append(w)
                    if dist[w] == dist[u] + 1:
                        sigma[w] += sigma[u]
            cof = {}
            for v in reversed(order):
                tot = 0.0
                for w in adj[v]:
                    if dist[w] == dist[v] + 1:
                        tot += cof[w]
                delta = sigma[v] * tot
                cof[v] = (1.0 + delta) / sigma[v]
                if v != s:
                    acc[v] += delta
        for v in members:
            bc[v] = acc[v] / ((nc - 1) * (nc - 2))
    return bc


def means(summary):
    """networkSummary's two numbers, (mean, size-weighted mean) of the components' maxima, formed exactly and rounded
    once; (0, 0) without a component"""
    if not summary:
        return 0.0, 0.0
    k = len(summary)
    return (float(sum(b for b, _ in summary) / k),
            float(sum(b * s for b, s in summary) / sum(s for _, s in summary)))


# ---- closed forms (Fractions; vertices are the local ids of the generators below) --------------------------------------
def star_values(leaves):
    """centre (local id 0) 1, leaves 0; nothing is scored below 4 vertices"""
    return [Fraction(1 if leaves >= 3 else 0)] + [Fraction(0)] * leaves


def path_values(n):
    if n <= 3:
        return [Fraction(0)] * n
    return [Fraction(2 * k * (n - 1 - k), (n - 1) * (n - 2)) for k in range(n)]


def clique_values(n):
    return [Fraction(0)] * n


def cycle_values(n):
    """every vertex the same: (n - 3) / (4 (n - 2)) for odd n, (n - 2) / (4 (n - 1)) for even n"""
    if n <= 3:
        return [Fraction(0)] * n
    return [Fraction(n - 3, 4 * (n - 2)) if n % 2 else Fraction(n - 2, 4 * (n - 1))] * n


def bipartite_values(a, b):
    """K_{a,b}, side A first: a vertex of A lies on 1/a of the shortest paths between every ordered pair of B"""
    n = a + b
    if n <= 3:
        return [Fraction(0)] * n
    d = (n - 1) * (n - 2)
    return [Fraction(b * (b - 1), a * d)] * a + [Fraction(a * (a - 1), b * d)] * b


# ---- bt_plan_kernel, restated ------------------------------------------------------------------------------------------
def plan(sizes_adj, small_max, lds_max):
    """sizes_adj: (n_c, adj_c) of every component of more than 3 vertices, adj_c = its adjacency entries (twice its
    edges).  Returns {K, K_big, K_glob, s, items}: how many components are scored, how many of them go to 256-thread
    items (n_c > small_max) and of those to the global-state path (n_c > lds_max), and per component the sources per
    item and the number of items.  lds_max <= 0 is the default."""
    small_max = min(max(int(small_max), 0), BT_SMALL_CAP)
    lds_max = BT_LDS_DEFAULT if lds_max <= 0 else min(int(lds_max), BT_LDS_DEFAULT)
    big = [(nc, adj) for nc, adj in sizes_adj if nc > small_max]
    work = float(sum(nc * (adj + nc) for nc, adj in big))      # integers far below 2^53: any order of addition
    target = max(work / BT_ITEMS, 1.0)
    s, items = [], []
    for nc, adj in sizes_adj:
        x = nc
        if nc > small_max:
            x = min(nc, max(1, int(math.ceil(target / float(adj + nc)))))
        s.append(x)
        items.append((nc + x - 1) // x)
    return {"K": len(sizes_adj), "K_big": len(big), "K_glob": sum(1 for nc, _ in big if nc > lds_max), "s": s,
            "items": items}


def sizes_adj(edges, n):
    return [(len(members), 2 * m) for members, m in components(edges, n)[0]]


# ---- generators ----------------------------------------------------------------------------------------------------------
def _finish(rng, pairs, relabel=None):
    """pairs [m, 2] -> relabelled, each orientation flipped with probability 1/2, permuted"""
    e = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if relabel is not None:
        e = np.asarray(relabel, dtype=np.int64)[e]
    swap = rng.random(e.shape[0]) < 0.5
    e[swap] = e[swap][:, ::-1]
    perm = rng.permutation(e.shape[0])
    return np.ascontiguousarray(e[perm]), perm


def has_repeated_pair(i, j=None):
    e = np.asarray(i).reshape(-1, 2) if j is None else np.stack([np.asarray(i), np.asarray(j)], axis=1)
    key = np.minimum(e[:, 0], e[:, 1]) * (int(e.max()) + 1 if e.size else 1) + np.maximum(e[:, 0], e[:, 1])
    return np.unique(key).size != key.size


def random_graph(seed, n, p, offsets, isolated=()):
    """G(n, p) over the vertices not in `isolated`, offsets drawn from `offsets` -> (i, j, o)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.triu_indices(n, 1)
    keep = rng.random(ii.size) < p
    for v in isolated:
        keep &= (ii != v) & (jj != v)
    e, _ = _finish(rng, np.stack([ii[keep], jj[keep]], axis=1))
    o = rng.choice(np.asarray(offsets, dtype=np.int64), size=e.shape[0])
    return e[:, 0].copy(), e[:, 1].copy(), o


def random_edges(seed, n, m, offsets):
    """exactly m distinct unordered pairs over n vertices -> (i, j, o)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.triu_indices(n, 1)
    pick = rng.choice(ii.size, size=m, replace=False)
    e, _ = _finish(rng, np.stack([ii[pick], jj[pick]], axis=1))
    o = rng.choice(np.asarray(offsets, dtype=np.int64), size=m)
    return e[:, 0].copy(), e[:, 1].copy(), o


def width_boundary_graph(n, n_off=5):
    """a sparse random graph over vertices 1 .. n-1 (0 isolated where n > 2) with the edge (n-2, n-1) at the last
    offset -> (i, j, o)"""
    i, j, o = random_graph(n, n, min(1.0, 3.0 / n), range(n_off), isolated=(0,) if n > 2 else ())
    keep = ~((np.minimum(i, j) == n - 2) & (np.maximum(i, j) == n - 1))
    return (np.concatenate([i[keep], [n - 1]]), np.concatenate([j[keep], [n - 2]]),
            np.concatenate([o[keep], [n_off - 1]]).astype(np.int64))


def hub_graph(n, hub_deg, second_deg, p, offsets, seed=0):
    """Vertex 0, the smallest id, is joined to 1 .. hub_deg, all higher; vertex 1 is joined to second_deg - 1 further
    vertices of 2 .. hub_deg and to every vertex above hub_deg, so it has at least second_deg higher neighbours of its
    own; every other pair of 1 .. hub_deg is an edge with probability p.  Ids 2 .. hub_deg are shuffled among
    themselves.  -> (i, j, o, n)"""
    rng = np.random.default_rng(seed)
    assert 2 <= hub_deg < n and second_deg <= n - 2
    pairs = {(0, v) for v in range(1, hub_deg + 1)}
    pairs |= {(1, v) for v in range(hub_deg + 1, n)}
    need = max(second_deg - (n - 1 - hub_deg), 0)
    pairs |= {(1, int(v)) for v in rng.choice(np.arange(2, hub_deg + 1), size=need, replace=False)}
    ii, jj = np.triu_indices(hub_deg, 1)
    keep = rng.random(ii.size) < p
    pairs |= {(int(a) + 1, int(b) + 1) for a, b in zip(ii[keep], jj[keep])}
    relabel = np.arange(n)
    relabel[2:hub_deg + 1] = 2 + rng.permutation(hub_deg - 1)
    e, _ = _finish(rng, sorted(pairs), relabel)
    o = rng.choice(np.asarray(offsets, dtype=np.int64), size=e.shape[0])
    return e[:, 0].copy(), e[:, 1].copy(), o, n


def tree_with_chords(rng, size, chords):
    """a random tree over `size` local ids plus up to `chords` further distinct pairs"""
    pairs = {(int(rng.integers(0, k)), k) for k in range(1, size)}
    for _ in range(chords):
        a, b = sorted(int(x) for x in rng.choice(size, size=2, replace=False))
        pairs.add((a, b))
    return sorted(pairs)


def path_with_chords(rng, size, chords):
    pairs = {(k, k + 1) for k in range(size - 1)}
    for _ in range(chords):
        a, b = sorted(int(x) for x in rng.choice(size, size=2, replace=False))
        pairs.add((a, b))
    return sorted(pairs)


def path(size):
    return [(k, k + 1) for k in range(size - 1)]


def star(leaves):
    return [(0, k) for k in range(1, leaves + 1)]


def clique(size):
    return [(a, b) for a in range(size) for b in range(a + 1, size)]


def cycle(size):
    return [(k, (k + 1) % size) for k in range(size)]


def bipartite(a, b):
    return [(x, a + y) for x in range(a) for y in range(b)]


def lattice(r, c):
    """the r x c grid graph, local id = row * c + column"""
    pairs = [(y * c + x, y * c + x + 1) for y in range(r) for x in range(c - 1)]
    return pairs + [(y * c + x, (y + 1) * c + x) for y in range(r - 1) for x in range(c)]


def hub_and_random(rng, size, extra):
    """local id 0 joined to every other vertex, plus `extra` further distinct pairs among the others"""
    pairs = {(0, k) for k in range(1, size)}
    while len(pairs) < size - 1 + extra:
        a, b = sorted(int(x) for x in rng.choice(np.arange(1, size), size=2, replace=False))
        pairs.add((a, b))
    return sorted(pairs)


def assemble(seed, parts):
    """parts: [(pairs over local ids 0 .. size-1, size)].  The disjoint union with ids shuffled -> (edges int64 [m, 2],
    n, ids) where ids[k][v] is the vertex that part k's local id v became."""
    rng = np.random.default_rng(seed)
    n = sum(size for _, size in parts)
    relabel = rng.permutation(n)
    pairs, ids, at = [], [], 0
    for local, size in parts:
        pairs += [(a + at, b + at) for a, b in local]
        ids.append(relabel[at:at + size])
        at += size
    e, _ = _finish(rng, pairs, relabel)
    return e, n, ids


def many_components_parts(seed, k, size_lo, size_hi, small=25):
    """k trees-with-chords of size_lo .. size_hi (> 3) vertices, the sizes drawn in runs so that many are equal, and
    `small` components of 1 .. 3 vertices, as parts for assemble()"""
    rng = np.random.default_rng(seed)
    assert size_lo > 3
    sizes = []
    while len(sizes) < k:
        sizes += [int(rng.integers(size_lo, size_hi + 1))] * int(rng.integers(1, 8))
    parts = [(tree_with_chords(rng, sz, int(rng.integers(0, sz))), sz) for sz in sizes[:k]]
    for _ in range(small):
        sz = int(rng.integers(1, 4))
        parts.append((path(sz), sz))
    return parts


def many_components(k, size_lo, size_hi, seed=0, small=25):
    """-> (edges [m, 2], n): k connected components of more than 3 vertices, and some of <= 3"""
    e, n, _ = assemble(seed + 1, many_components_parts(seed, k, size_lo, size_hi, small))
    return e, n


def two_sets_many_bridges(a, b, bridges, seed=0):
    """offset 0: a star over a vertices and a star over b vertices; offset 1: `bridges` distinct edges, every one
    between the two sets, so the whole batch makes exactly one link.  -> (i, j, o, n)"""
    rng = np.random.default_rng(seed)
    assert bridges <= a * b
    n = a + b
    pairs = star(a - 1) + [(a, a + k) for k in range(1, b)]
    pick = rng.choice(a * b, size=bridges, replace=False)
    pairs += [(int(x) // b, a + int(x) % b) for x in pick]
    o = np.array([0] * (n - 2) + [1] * bridges, dtype=np.int64)
    e, perm = _finish(rng, pairs, rng.permutation(n))
    return e[:, 0].copy(), e[:, 1].copy(), o[perm], n


def triangle_orderings():
    """13 disjoint triangles on vertices a < b < c = 3k, 3k + 1, 3k + 2, one for every weak ordering of the offsets of
    (ab, bc, ac): 1 with all equal, 6 with two values, 6 with three; n_off = 3.  -> (i, j, o, n, patterns)"""
    patterns = [(x, y, z) for x in range(3) for y in range(3) for z in range(3)
                if set((x, y, z)) == set(range(max(x, y, z) + 1))]
    assert len(patterns) == 13
    rng = np.random.default_rng(13)
    pairs, o = [], []
    for k, (ab, bc, ac) in enumerate(patterns):
        a, b, c = 3 * k, 3 * k + 1, 3 * k + 2
        pairs += [(a, b), (b, c), (a, c)]
        o += [ab, bc, ac]
    e, perm = _finish(rng, pairs)
    return e[:, 0].copy(), e[:, 1].copy(), np.array(o, dtype=np.int64)[perm], 39, patterns


def map_values(n, ids, per_part):
    """per-part closed-form lists (or None) -> Fractions per vertex, None where no closed form was given"""
    out = [None] * n
    for part_ids, vals in zip(ids, per_part):
        if vals is not None:
            for v, x in zip(part_ids.tolist(), vals):
                out[v] = x
    return out


# ---- the designed cases (built once; tests/test_network_shapes_host.py proves each reaches its branch) ------------------
import functools  # noqa: E402

HIGH_OFFSETS = (0, 1, 511, 512, 513, 1021, 1022)


@functools.lru_cache(maxsize=None)
def case_offsets_up_to_1022():
    """n = 200, p = 0.15, n_off = 1023: offsets around the top bit of the 10-bit field, the last two, and 30 across the
    whole range -> (i, j, o, n, n_off)"""
    rng = np.random.default_rng(1022)
    used = np.unique(np.concatenate([np.array(HIGH_OFFSETS), rng.choice(1023, size=30, replace=False)]))
    i, j, o = random_graph(1023, 200, 0.15, used)
    return i, j, o, 200, 1023


@functools.lru_cache(maxsize=None)
def case_hub():
    """hub_graph(700, 620, 220, 0.05) over 12 offsets of 40 -> (i, j, o, n, n_off)"""
    offsets = (0, 1, 2, 5, 9, 14, 20, 27, 31, 36, 38, 39)
    i, j, o, n = hub_graph(700, 620, 220, 0.05, offsets, seed=7)
    return i, j, o, n, 40


@functools.lru_cache(maxsize=None)
def case_bridges(a, b, bridges):
    i, j, o, n = two_sets_many_bridges(a, b, bridges, seed=a + bridges)
    return i, j, o, n, 2


@functools.lru_cache(maxsize=None)
def case_multi_source():
    """300 components of 4 .. 9 vertices and one sparse one of 120 -> (edges, n)"""
    rng = np.random.default_rng(120)
    parts = many_components_parts(300, 300, 4, 9) + [(tree_with_chords(rng, 120, 30), 120)]
    e, n, _ = assemble(301, parts)
    return e, n


@functools.lru_cache(maxsize=None)
def case_many(k):
    """k components of 4 .. 6 vertices, many of equal size, and some of <= 3 -> (edges, n)"""
    return many_components(k, 4, 6, seed=k)


@functools.lru_cache(maxsize=None)
def case_star(leaves=300):
    """-> (edges, n, exact values)"""
    e, n, ids = assemble(leaves, [(star(leaves), leaves + 1), (path(3), 3)])
    return e, n, map_values(n, ids, [star_values(leaves), path_values(3)])


@functools.lru_cache(maxsize=None)
def case_hub_component():
    """300 vertices, one of them joined to all the others, about 900 edges, and a 5-vertex path -> (edges, n)"""
    rng = np.random.default_rng(299)
    e, n, _ = assemble(300, [(hub_and_random(rng, 300, 600), 300), (path(5), 5)])
    return e, n


@functools.lru_cache(maxsize=None)
def case_small_cap():
    """a 256-vertex path, a 257-vertex path and a 16 x 16 lattice -> (edges, n, exact values where a closed form gives
    them, else None)"""
    e, n, ids = assemble(256, [(path(256), 256), (path(257), 257), (lattice(16, 16), 256)])
    return e, n, map_values(n, ids, [path_values(256), path_values(257), None])


BOUNDARY_SIZES = (64, 65, 100, 101)          # bt_small_max = 64, bt_lds_max = 100


@functools.lru_cache(maxsize=None)
def case_path_boundaries():
    """components of exactly small_max, small_max + 1, lds_max and lds_max + 1 vertices, each a path plus a few chords"""
    rng = np.random.default_rng(64100)
    e, n, _ = assemble(101, [(path_with_chords(rng, sz, 5), sz) for sz in BOUNDARY_SIZES])
    return e, n


@functools.lru_cache(maxsize=None)
def case_before_first_edge():
    """n_off = 5, no edge before offset 2 -> (edges, o, n, n_off)"""
    e, n = many_components(12, 4, 10, seed=5, small=6)
    o = np.random.default_rng(52).choice(np.array([2, 3, 4]), size=e.shape[0]).astype(np.int64)
    return e, o, n, 5


@functools.lru_cache(maxsize=None)
def case_reorder():
    """12 offsets: 30 components of 4 .. 12 vertices that grow from their own edges (offsets 0 .. 5) and are then joined
    by bridges (offsets 4 .. 11), so sizes overtake one another and the (size descending, root) order reshuffles
    -> (edges, o, n, n_off)"""
    rng = np.random.default_rng(12)
    parts = many_components_parts(77, 30, 4, 12, small=8)
    e, n, ids = assemble(78, parts)
    o = rng.integers(0, 6, size=e.shape[0])
    big = [x for x in ids if x.size > 3]
    pairs, po = [], []
    for k in range(16):
        a, b = rng.choice(len(big), size=2, replace=False)
        pairs.append((int(rng.choice(big[a])), int(rng.choice(big[b]))))
        po.append(4 + k % 8)
    keep = [k for k, p in enumerate(pairs) if pairs.index(p) == k and (p[1], p[0]) not in pairs[:k]]
    e = np.concatenate([e, np.array([pairs[k] for k in keep], dtype=np.int64)])
    o = np.concatenate([o, np.array([po[k] for k in keep])]).astype(np.int64)
    perm = rng.permutation(e.shape[0])
    return np.ascontiguousarray(e[perm]), o[perm], n, 12


@functools.lru_cache(maxsize=None)
def exact(case, *args):
    """brandes_exact of a case's graph, computed once: (values float64, summary)"""
    e, n = case(*args)[:2]
    return brandes_exact(e, n)


@functools.lru_cache(maxsize=None)
def exact_sweep(case):
    """brandes_exact of every G_t of a sweep case (edges, o, n, n_off), computed once: [(values, summary)] per t"""
    e, o, n, n_off = case()
    return [brandes_exact(e[o <= t], n) for t in range(n_off)]
