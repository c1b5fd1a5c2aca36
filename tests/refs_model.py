"""The reference-picking rule (include/ppk.h "Reference genomes of a cluster network") restated in
numpy and Python integers, step for step: components, clique pruning or the fast rank test, repair, outputs.  Beside
it `check_properties`, which shares no code with the restatement (its own union-find over dictionaries, neighbour
sets instead of bit rows, clique membership recomputed from the flags it is handed), and the graph builders of the
tests with the claims they make.
"""
import numpy as np

COUNT_NAMES = ("references", "reference_edges", "components", "cliques_removed", "from_cliques", "from_small",
               "added_by_repair", "components_repaired")


# ---- the restatement ---------------------------------------------------------------------------------------------

def _labels(edges, n):
    """label[v] = the smallest vertex of v's component (array union-find, the larger root under the smaller)"""
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(n)], dtype=np.int64)


def _rows(verts, edges_in):
    """component-local bit rows as Python integers: bit l of row k <-> verts[k] and verts[l] adjacent"""
    local = {v: k for k, v in enumerate(verts)}
    rows = [0] * len(verts)
    for a, b in edges_in:
        rows[local[a]] |= 1 << local[b]
        rows[local[b]] |= 1 << local[a]
    return rows


def _low(x):
    return (x & -x).bit_length() - 1


def pick_refs(edges, n, existing=None, merged=None, fast=False):
    """-> (is_ref uint8 [n], ref_edges int64 [k, 2], counts dict with COUNT_NAMES)"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n = int(n)
    if edges.size and (edges.min() < 0 or edges.max() >= n or (edges[:, 0] == edges[:, 1]).any()):
        raise ValueError("bad edge")
    is_ref = np.zeros(n, dtype=np.uint8) if existing is None else (np.asarray(existing) != 0).astype(np.uint8)
    merged = np.zeros(n, dtype=bool) if merged is None else np.asarray(merged) != 0
    n_existing = int(is_ref.sum())
    label = _labels(edges, n)
    comps = {}
    for v in range(n):
        comps.setdefault(int(label[v]), []).append(v)
    comp_edges = {r: [] for r in comps}
    for a, b in edges.tolist():
        comp_edges[int(label[a])].append((a, b))
    rows_of = {r: _rows(comps[r], comp_edges[r]) for r in comps if len(comps[r]) >= 3}
    cliques = pick_a = pick_b = 0
    for r, verts in comps.items():
        size = len(verts)
        if fast:
            if not is_ref[verts].any():
                for v in verts[:size // 10 + 1]:
                    is_ref[v] = 1
                    pick_a += 1
            m_here = [v for v in verts if merged[v]]
            if m_here:
                for v in m_here[:len(m_here) // 3 + 1]:
                    if not is_ref[v]:
                        is_ref[v] = 1
                        pick_b += 1
            continue
        if size <= 2:
            if not is_ref[verts[0]]:
                is_ref[verts[0]] = 1
                pick_b += 1
            continue
        rows = rows_of[r]
        ref = sum(1 << k for k, v in enumerate(verts) if is_ref[v])
        R = (1 << size) - 1
        while R:
            s = _low(R)
            K, C = 1 << s, rows[s] & R
            while C:
                v = _low(C)
                K |= 1 << v
                C &= rows[v]
            if not K & ref:
                ref |= 1 << s
                is_ref[verts[s]] = 1
                pick_a += 1
            R &= ~K
            cliques += 1

    # repair
    ref_label = _labels(edges[(is_ref[edges[:, 0]] != 0) & (is_ref[edges[:, 1]] != 0)], n) if len(edges) else np.arange(n)
    before = is_ref.copy()
    repaired = 0
    for r, verts in comps.items():
        refs = [v for v in verts if before[v]]
        if not refs:
            continue
        r0 = refs[0]
        strays = [v for v in refs if ref_label[v] != ref_label[r0]]
        if not strays:
            continue
        repaired += 1
        rows, local = rows_of[r], {v: k for k, v in enumerate(verts)}
        parent = {local[r0]: -1}
        frontier = 1 << local[r0]
        visited = frontier
        while frontier:
            nxt = 0
            for l in range(len(verts)):
                if not (visited >> l) & 1 and rows[l] & frontier:
                    parent[l] = _low(rows[l] & frontier)
                    nxt |= 1 << l
            visited |= nxt
            frontier = nxt
        for v in strays:
            p = local[v]
            while p != local[r0]:
                p = parent[p]
                is_ref[verts[p]] = 1

    rank = np.cumsum(is_ref, dtype=np.int64) - is_ref
    keep = (is_ref[edges[:, 0]] != 0) & (is_ref[edges[:, 1]] != 0) if len(edges) else np.zeros(0, dtype=bool)
    ref_edges = rank[edges[keep]].reshape(-1, 2)
    n_refs = int(is_ref.sum())
    counts = dict(zip(COUNT_NAMES, (n_refs, len(ref_edges), len(comps), cliques, pick_a, pick_b,
                                    n_refs - n_existing - pick_a - pick_b, repaired)))
    return is_ref, ref_edges, counts


# ---- the independent checker ---------------------------------------------------------------------------------------

def _sets(edges, n, only=None):
    """vertex -> representative, by a dictionary union-find that links under the representative first seen"""
    rep = {v: v for v in range(n)}

    def top(x):
        path = []
        while rep[x] != x:
            path.append(x)
            x = rep[x]
        for y in path:
            rep[y] = x
        return x
    for a, b in edges:
        if only is None or (a in only and b in only):
            ta, tb = top(a), top(b)
            if ta != tb:
                rep[tb] = ta
    return {v: top(v) for v in range(n)}


def greedy_cliques(members, nbrs):
    """the cliques the rule removes from one component, as sets, by neighbour sets"""
    left, out = set(members), []
    while left:
        s = min(left)
        clique, cand = {s}, nbrs[s] & left
        while cand:
            v = min(cand)
            clique.add(v)
            cand = cand & nbrs[v]
        out.append(clique)
        left -= clique
    return out


def check_properties(edges, n, is_ref, ref_edges=None, clique_mode=True, own_cliques=True):
    """P1 (clique mode only), P2, P3 of DESIGN.md 3.25 on a returned flag array (and edge list): the list of
    violations, empty when all hold.  own_cliques=False, for a pick made over another clique order (the
    reference's): P1 as what it implies whichever cliques were removed -- the references dominate G."""
    edges = [tuple(e) for e in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist()]
    refs = {v for v in range(n) if is_ref[v]}
    comp = _sets(edges, n)
    members = {}
    for v in range(n):
        members.setdefault(comp[v], set()).add(v)
    nbrs = {v: set() for v in range(n)}
    for a, b in edges:
        nbrs[a].add(b)
        nbrs[b].add(a)
    bad = []
    if clique_mode:
        for c, mem in members.items():
            if len(mem) <= 2:
                if min(mem) not in refs:
                    bad.append("P1: small component %s lacks its lowest vertex" % sorted(mem))
                continue
            for clique in greedy_cliques(mem, nbrs) if own_cliques else ():
                if not clique & refs:
                    bad.append("P1: clique %s holds no reference" % sorted(clique))
        for v in range(n):                                   # ... and so the references dominate G
            if v not in refs and not nbrs[v] & refs:
                bad.append("P1: vertex %d has no reference neighbour" % v)
    among = _sets(edges, n, only=refs)
    for c, mem in members.items():
        if len({among[v] for v in mem & refs}) > 1:
            bad.append("P2: the references of component %d are not connected" % c)
    if ref_edges is not None:
        order = sorted(refs)
        want = [(a, b) for a, b in edges if a in refs and b in refs]
        got = [(order[a], order[b]) for a, b in np.asarray(ref_edges).reshape(-1, 2).tolist()]
        if got != want:
            bad.append("reference edges are not the stream's, renumbered by rank")
        for a, b in got:
            if comp[a] != comp[b]:
                bad.append("P3: reference edge (%d, %d) joins two components" % (a, b))
    return bad


# ---- builders ------------------------------------------------------------------------------------------------------

def clique(k, base=0):
    return [(base + a, base + b) for a in range(k) for b in range(a + 1, k)]


def path(k, base=0):
    return [(base + a, base + a + 1) for a in range(k - 1)]


def star(leaves, centre_lowest=True):
    """leaves + 1 vertices"""
    c = 0 if centre_lowest else leaves
    return [(c, v) for v in range(leaves + 1) if v != c]


def random_graph(k, density, seed, base=0):
    """a CONNECTED graph on k vertices: a random spanning path plus each other pair with the given density"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(k)
    have = {(min(a, b), max(a, b)) for a, b in zip(perm[:-1].tolist(), perm[1:].tolist())}
    iu = np.triu_indices(k, 1)
    take = rng.random(len(iu[0])) < density
    have |= set(zip(iu[0][take].tolist(), iu[1][take].tolist()))
    return [(base + a, base + b) for a, b in sorted(have)]


def dumbbell(k=20, bridge=6):
    """two K_k joined by a path of `bridge` vertices: 2 k + bridge vertices.  The two cliques give one reference
    each, `bridge` apart -- the repair has to join them."""
    e = clique(k) + clique(k, k + bridge)
    chain = [k - 1] + list(range(k, k + bridge)) + [k + bridge]
    return e + list(zip(chain[:-1], chain[1:])), 2 * k + bridge


def far_existing(hops=5):
    """a path of hops + 1 vertices whose two ends are existing references: whatever the pruning picks in between,
    the repair adds the rest, and all hops - 1 vertices between the ends come out as references"""
    n = hops + 1
    existing = np.zeros(n, dtype=np.uint8)
    existing[[0, hops]] = 1
    return path(n), n, existing


def planted(n, strains, p_in, p_out_edges, seed):
    """strains of equal size in shuffled vertex order, within-strain density p_in, plus a few cross-strain edges"""
    rng = np.random.default_rng(seed)
    strain = rng.permutation(n) % strains
    iu = np.triu_indices(n, 1)
    same = strain[iu[0]] == strain[iu[1]]
    take = same & (rng.random(len(iu[0])) < p_in)
    e = np.stack([iu[0][take], iu[1][take]], axis=1)
    if p_out_edges:
        cross = np.flatnonzero(~same)
        pick = rng.choice(cross, size=p_out_edges, replace=False)
        e = np.concatenate([e, np.stack([iu[0][pick], iu[1][pick]], axis=1)])
    return e.astype(np.int64), n


def shifted(parts):
    """[(edges, n), ...] side by side -> (edges int64 [m, 2], n)"""
    out, base = [], 0
    for e, k in parts:
        out += [(a + base, b + base) for a, b in e]
        base += k
    return np.asarray(out, dtype=np.int64).reshape(-1, 2), base
