"""Exact references for the sampled-source betweenness and the whole-graph values (ppk_network_summary_sampled*,
DESIGN.md 3.8), on top of tests/network_model.py.

  sample_key / sample_of   the [EXT] sampling rule, restated: the k vertices of a component with the smallest
                           (h(seed, v), v), h = the high 32 bits of fmix64(seed + (v + 1) * 0x9E3779B97F4A7C15)
  delta_sums               Brandes restricted to a source list: sigma in Python ints, delta in Fractions
  sampled_exact            every vertex's value and the per-component summary, in either normalisation, each value the
                           correctly rounded exact one
  scaled_float             the device's floating-point statement of the scale, operation by operation
  plan                     bt_plan_kernel's arithmetic with source counts

No device, no poppunk_amd import: tests/test_network_sample_host.py checks this module on the CPU and
tests/test_gpu_network_sample.py uses it."""
import functools
import math
from collections import deque
from fractions import Fraction

import numpy as np

import network_model as nm

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def fmix64(z):
    """splitmix64's finaliser on a Python int (mod 2^64)"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_key(seed, v):
    return fmix64(seed + (v + 1) * GOLDEN) >> 32


def sample_of(component_vertices, k, seed):
    """the sources of a component: all of it when it has at most k vertices, else its k vertices of smallest
    (sample_key, id); ascending ids (the order of the device's local ids)"""
    members = sorted(int(v) for v in component_vertices)
    if len(members) <= k:
        return members
    return sorted(sorted(members, key=lambda v: (sample_key(seed, v), v))[:k])


def components_min(edges, n, min_nc):
    """(sorted member lists of the components of at least min_nc vertices, largest first then by smallest member;
    adjacency lists)"""
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
        if len(members) >= min_nc:
            out.append(sorted(members))
    out.sort(key=lambda c: (-len(c), c[0]))
    return out, adj


def delta_sums(adj, members, sources):
    """{v: sum over s in sources of delta_s(v)} for the vertices of one component, exact"""
    acc = dict.fromkeys(members, Fraction(0))
    for s in sources:
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
    return acc


def scale_exact(nc, k, n_all=None):
    """the factor on the sum of deltas: 1 / ((n_c - 1)(n_c - 2)) with every source, n_c / (k (n_c - 1)(n_c - 2)) with
    k < n_c of them (networkx 3.4.2's _rescale); n_all: the whole graph's (n - 1)(n - 2) in place of the component's"""
    d = (nc - 1) * (nc - 2) if n_all is None else (n_all - 1) * (n_all - 2)
    return Fraction(nc, k * d) if nc > k else Fraction(1, d)


def scaled_float(s, nc, k, n_all=None):
    """bt_reduce_kernel's statement in float64, S the float sum of the partials:
         every source   S / (double(nc - 1) * double(nc - 2))
         k < nc         (S * double(nc)) / (double(k) * (double(nc - 1) * double(nc - 2)))
    and with n_all the product double(n_all - 1) * double(n_all - 2) in place of the component's."""
    m = nc if n_all is None else n_all
    prod = float(m - 1) * float(m - 2)
    if nc > k:
        return (float(s) * float(nc)) / (float(k) * prod)
    return float(s) / prod


def sampled_exact(edges, n, k, seed, whole=False, fractions=False):
    """-> (values, summary, samples).  values float64 [n]: per-component normalisation over the components of more than
    3 vertices, or (whole) networkx's betweenness_centrality(G) normalisation over those of at least 3; each the
    correctly rounded exact value (Fractions with fractions=True).  summary = [(exact maximum in the component's own
    normalisation, size)] per component of more than 3 vertices, whichever `whole`.  samples = {smallest member: source
    list} of every component that was sampled (n_c > k)."""
    comps, adj = components_min(edges, n, 3 if whole else 4)
    bc = [Fraction(0)] * n
    summary, samples = [], {}
    for members in comps:
        nc = len(members)
        sources = sample_of(members, k, seed)
        if nc > k:
            samples[members[0]] = sources
        acc = delta_sums(adj, members, sources)
        own = scale_exact(nc, k)
        if nc > 3:
            summary.append((max(acc[v] for v in members) * own, nc))
        use = scale_exact(nc, k, n) if whole else own
        for v in members:
            bc[v] = acc[v] * use
    if fractions:
        return bc, summary, samples
    return np.array([float(x) for x in bc], dtype=np.float64), summary, samples


K_ALL = 1 << 31            # "every source": no component is larger


def whole_exact(edges, n, norm=True):
    """vertex_betweenness(G, norm) with every source: networkx's betweenness_centrality(G, normalized=norm)"""
    bc, _, _ = sampled_exact(edges, n, K_ALL, 0, whole=True, fractions=True)
    if not norm:
        bc = [x * (n - 1) * (n - 2) / 2 for x in bc]
    return np.array([float(x) for x in bc], dtype=np.float64)


def plan(sizes_adj, small_max, lds_max, k):
    """nm.plan with source counts: work = sources x (adjacency + n_c), items = ceil(sources / s), sources = min(n_c,
    k).  Adds "sources" to the returned dict."""
    small_max = min(max(int(small_max), 0), nm.BT_SMALL_CAP)
    lds_max = nm.BT_LDS_DEFAULT if lds_max <= 0 else min(int(lds_max), nm.BT_LDS_DEFAULT)
    big = [(nc, adj) for nc, adj in sizes_adj if nc > small_max]
    work = float(sum(min(nc, k) * (adj + nc) for nc, adj in big))
    target = max(work / nm.BT_ITEMS, 1.0)
    s, items, sources = [], [], []
    for nc, adj in sizes_adj:
        ns = min(nc, k)
        x = ns
        if nc > small_max:
            x = min(ns, max(1, int(math.ceil(target / float(adj + nc)))))
        s.append(x)
        sources.append(ns)
        items.append((ns + x - 1) // x)
    return {"K": len(sizes_adj), "K_big": len(big), "K_glob": sum(1 for nc, _ in big if nc > lds_max), "s": s,
            "items": items, "sources": sources}


def sizes_adj_min(edges, n, min_nc=4):
    comps, adj = components_min(edges, n, min_nc)
    return [(len(c), sum(len(adj[v]) for v in c)) for c in comps]


def bar_ratio(got, want):
    """max |got - want| / max(1e-12 |want|, 1e-15) (DESIGN.md 3.8's bar); values that are exactly 0 or 1 must be equal"""
    got = np.asarray(got, dtype=np.float64).ravel()
    want = np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    exact = (want == 0.0) | (want == 1.0)
    assert np.array_equal(got[exact], want[exact]), np.abs(got[exact] - want[exact]).max()
    if not got.size:
        return 0.0
    return float((np.abs(got - want) / np.maximum(1e-12 * np.abs(want), 1e-15)).max())


# ---- the designed cases (built once; tests/test_network_sample_host.py proves each reaches its branch) ----------------
RULE_K = 100
RULE_SIZES = (99, 100, 101)


@functools.lru_cache(maxsize=None)
def case_rule_boundary(size):
    """one component of `size` vertices, a path with 5 chords, ids shuffled, and an isolated pair -> (edges, n)"""
    rng = np.random.default_rng(9000 + size)
    e, n, _ = nm.assemble(size, [(nm.path_with_chords(rng, size, 5), size), (nm.path(2), 2)])
    return e, n


CAP_SIZES = (64, 65, 66)


@functools.lru_cache(maxsize=None)
def case_cap():
    """components of 64, 65 and 66 vertices (trees with chords) around the one-wave cap -> (edges, n)"""
    rng = np.random.default_rng(646566)
    e, n, _ = nm.assemble(66, [(nm.tree_with_chords(rng, sz, 12), sz) for sz in CAP_SIZES])
    return e, n


STAR_K = 7


@functools.lru_cache(maxsize=None)
def case_star():
    """nm.case_star()'s 300-leaf star (and 3-path) -> (edges, n, centre)"""
    e, n, exact = nm.case_star()
    centre = [v for v, x in enumerate(exact) if x == 1][0]
    return e, n, centre


@functools.lru_cache(maxsize=None)
def star_seeds():
    """(seed with the centre in the 7-vertex sample, seed with it out): the first of each, counting from 0"""
    e, n, centre = case_star()
    comps, _ = components_min(e, n, 4)
    seed_in = seed_out = None
    for seed in range(10000):
        inside = centre in sample_of(comps[0], STAR_K, seed)
        if inside and seed_in is None:
            seed_in = seed
        if not inside and seed_out is None:
            seed_out = seed
        if seed_in is not None and seed_out is not None:
            return seed_in, seed_out
    raise AssertionError("no seed found")


WHOLE_N = 40


@functools.lru_cache(maxsize=None)
def case_whole():
    """40 vertices: 5 isolated, a pair, two 3-paths, a triangle, a 4-path and a 20-vertex part -> (edges, n, ids):
    ids[k] = the vertices of part k in the order above (the isolated vertices one part each)"""
    rng = np.random.default_rng(40)
    parts = [([], 1)] * 5 + [(nm.path(2), 2), (nm.path(3), 3), (nm.path(3), 3), (nm.clique(3), 3), (nm.path(4), 4),
                             (nm.tree_with_chords(rng, 20, 8), 20)]
    e, n, ids = nm.assemble(41, parts)
    assert n == WHOLE_N
    return e, n, ids


@functools.lru_cache(maxsize=None)
def exact(case, k, seed, whole=False, *args):
    """sampled_exact of a case's graph (its first two returns are edges, n), computed once"""
    e, n = case(*args)[:2]
    return sampled_exact(e, n, k, seed, whole)


@functools.lru_cache(maxsize=None)
def exact_sweep(case, k, seed):
    """sampled_exact of every G_t of a sweep case (edges, o, n, n_off), computed once"""
    e, o, n, n_off = case()
    return [sampled_exact(e[o <= t], n, k, seed) for t in range(n_off)]


# ---- poppunk_assign --betweenness, restated (PopPUNK/assign.py:646-651) -----------------------------------------------
def betweenness_table(query_names, query_values):
    """the text the reference prints: the header, then the queries by descending value, ties in their input order"""
    from operator import itemgetter
    out = "query\tbetweenness\n"
    for name, value in sorted(zip(query_names, query_values), key=itemgetter(1), reverse=True):
        out += f"{name}\t{value}\n"
    return out
