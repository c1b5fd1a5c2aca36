"""Neighbour-joining trees on the device (ppk_nj_dev, engine.nj_dev, trees.generate_nj_tree):
bit for bit against the same-rule restatement (tests/test_nj_host.py), tree recovery on additive matrices, real
synthetic distances, every input form, bad entries and repeatability.  Sizes are bounded (n <= 10 000, whose join
loop is n - 2 launches pairs), so a wrong kernel fails rather than hangs."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, synth, trees  # noqa: E402
from test_nj_host import nj_biopython_form, nj_same_rule  # noqa: E402

DEV = "cuda:0"


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def device_nj(D):
    join, ln = engine.nj_dev(torch.as_tensor(np.ascontiguousarray(D, dtype=np.float32), device=DEV))
    return join.cpu().numpy(), ln.cpu().numpy()


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))


def dyadic(n, seed, hi=2048):
    rng = np.random.default_rng(seed)
    A = rng.integers(0, hi, size=(n, n)).astype(np.float32) / np.float32(1024)
    return np.tril(A, -1) + np.tril(A, -1).T


def condensed(D):
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    return np.ascontiguousarray(D[iu], dtype=np.float32)


@pytest.mark.parametrize("n", [3, 4, 5, 17, 64, 257, 1000])
def test_dyadic_bit_for_bit(n):
    D = dyadic(n, seed=n)
    assert_same(device_nj(D), nj_same_rule(D))


@pytest.mark.parametrize("n", [4, 50, 300])
def test_designed_ties(n):
    flat = np.full((n, n), 0.5, dtype=np.float32)
    assert_same(device_nj(flat), nj_same_rule(flat))
    # blocks: 1 inside a block of 7, 3 between blocks (Q ties inside every block and between blocks)
    blk = np.arange(n) // 7
    B = np.where(blk[:, None] == blk[None, :], 1.0, 3.0).astype(np.float32)
    assert_same(device_nj(B), nj_same_rule(B))
    # zeros and negative zeros (equal Q of either sign)
    Z = np.where((np.arange(n)[:, None] + np.arange(n)[None, :]) % 2 == 0, -0.0, 0.0).astype(np.float32)
    assert_same(device_nj(Z), nj_same_rule(Z))


def random_tree(n, seed):
    """A random rooted binary tree of n leaves with dyadic branch lengths k/1024, k in 1..64 (every path sum exact in
    float32), and its patristic matrix.  Returns (D float32 [n, n], splits {canonical leaf-hash: length})."""
    rng = np.random.default_rng(seed)
    active = list(range(n))
    children, length = {}, {}
    nxt = n
    while len(active) > 1:
        i, j = sorted(rng.choice(len(active), 2, replace=False))[::-1]
        a, b = active.pop(i), active.pop(j)
        children[nxt] = (a, b)
        length[a] = int(rng.integers(1, 65)) / 1024.0
        length[b] = int(rng.integers(1, 65)) / 1024.0
        active.append(nxt)
        nxt += 1
    root = active[0]
    depth = {root: 0.0}
    members = {}
    order = [root]
    for v in order:
        for c in children.get(v, ()):
            depth[c] = depth[v] + length[c]
            order.append(c)
    D = np.zeros((n, n), dtype=np.float64)
    for v in reversed(order):
        if v < n:
            members[v] = np.array([v])
            continue
        a, b = children[v]
        L, R = members.pop(a), members.pop(b)
        dl = np.array([depth[x] for x in L]) - depth[v]
        dr = np.array([depth[x] for x in R]) - depth[v]
        D[np.ix_(L, R)] = dl[:, None] + dr[None, :]
        D[np.ix_(R, L)] = D[np.ix_(L, R)].T
        members[v] = np.concatenate([L, R])
    Df = D.astype(np.float32)
    assert np.array_equal(Df.astype(np.float64), D)
    # splits of the unrooted tree: the root's two edges are one split
    h = np.random.default_rng(seed + 1).integers(1, 2**63, size=n, dtype=np.int64).astype(np.uint64)
    total = np.bitwise_xor.reduce(h)
    sub = {}
    for v in reversed(order):
        sub[v] = h[v] if v < n else sub[children[v][0]] ^ sub[children[v][1]]
    splits = {}
    for v in order[1:]:
        key = int(min(sub[v], sub[v] ^ total))
        splits[key] = splits.get(key, 0.0) + length[v]
    return Df, splits, h, total


def device_splits(join, lens, n, h, total):
    t = trees.tree_from_joins(join, lens, n)
    sub = [np.uint64(0)] * len(t.children)
    for v in trees._postorder(t):
        if v < n:
            sub[v] = h[v]
        else:
            acc = np.uint64(0)
            for c in t.children[v]:
                acc ^= sub[c]
            sub[v] = acc
    splits = {}
    for v in range(len(t.children)):
        if v == t.root:
            continue
        key = int(min(sub[v], sub[v] ^ total))
        splits[key] = splits.get(key, 0.0) + t.length[v]
    return splits


@pytest.mark.parametrize("n", [50, 600, 10_000])
def test_additive_tree_recovered(n):
    D, want, h, total = random_tree(n, seed=n)
    t0 = time.time()
    join, lens = engine.nj_dev(torch.as_tensor(D, device=DEV))
    torch.cuda.synchronize()
    assert time.time() - t0 < 60
    got = device_splits(join.cpu().numpy(), lens.cpu().numpy(), n, h, total)
    assert set(got) == set(want)
    err = max(abs(got[k] - want[k]) for k in want)
    assert err < 1e-9


@pytest.fixture(scope="module")
def synth_dist():
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(2000, kmers, cluster_size=50, seed=11)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    return dist


@pytest.mark.parametrize("n", [300, 2000])
def test_synthetic_distances(synth_dist, n):
    sq = engine.long_to_square_dev(synth_dist, 0, 2000)[:n, :n].contiguous()
    D = sq.cpu().numpy()
    got = engine.nj_dev(sq)
    got = (got[0].cpu().numpy(), got[1].cpu().numpy())
    same = nj_same_rule(D)
    assert_same(got, same)
    # against Biopython's recomputed row sums: the same joins up to the first step whose Q margin is within
    # 1e-9 |Q| in either restatement (after it the two may legitimately part)
    bio = nj_biopython_form(D)
    steps = first_near_tie(D)
    assert np.array_equal(got[0][:steps], bio[0][:steps])
    np.testing.assert_allclose(got[1][:steps], bio[1][:steps], rtol=0, atol=1e-9)


def first_near_tie(D):
    """The first join whose best and second-best Q (same-rule state, distinct pairs) are within 1e-9 |Q|."""
    from test_nj_host import _symmetric
    M = _symmetric(D)
    n = M.shape[0]
    alive = np.ones(n, dtype=bool)
    S = np.zeros(n)
    for j in range(n):
        S = S + M[:, j]
    r, t = n, 0
    while r > 2:
        act = np.flatnonzero(alive)
        sub = M[np.ix_(act, act)]
        nd = S[act] / (r - 2)
        Q = (sub - nd[:, None]) - nd[None, :]
        Q[np.triu_indices(r)] = np.inf
        flat = np.sort(np.partition(Q.ravel(), 1)[:2])
        if flat[1] - flat[0] <= 1e-9 * abs(flat[0]):
            return t
        ia, ib = divmod(int(np.argmin(Q)), r)
        a, b = act[ia], act[ib]
        dab = M[a, b]
        k = act[(act != a) & (act != b)]
        dak, dbk = M[a, k], M[b, k]
        dn = ((dak + dbk) - dab) / 2.0
        S[k] = ((S[k] - dak) - dbk) + dn
        S[b] = ((S[a] + S[b]) - float(r) * dab) / 2.0
        M[b, k] = dn
        M[k, b] = dn
        alive[a] = False
        r, t = r - 1, t + 1
    return n - 1


def test_every_input_form_and_garbage_ignored():
    n = 700
    D = dyadic(n, seed=5)
    want = nj_same_rule(D)
    G = D.copy()
    iu = np.triu_indices(n, 0)
    G[iu] = np.random.default_rng(1).random(len(iu[0])).astype(np.float32) * 100 - 50   # upper triangle + diagonal
    G[0, 1] = np.nan
    G[2, 2] = np.inf
    assert_same(engine.nj(G), want)
    assert_same(device_nj(G), want)
    v = condensed(D)
    assert_same(tuple(x.cpu().numpy() for x in engine.nj_dev(torch.as_tensor(v, device=DEV))), want)
    for col in (0, 1):
        two = np.random.default_rng(col).random((len(v), 2)).astype(np.float32)
        two[:, col] = v
        got = engine.nj_dev(torch.as_tensor(two, device=DEV), n=n, col=col)
        assert_same(tuple(x.cpu().numpy() for x in got), want)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_entry_named(bad):
    D = dyadic(40, seed=2)
    D[31, 17] = bad
    with pytest.raises(RuntimeError) as e:
        device_nj(D)
    assert "(31, 17)" in str(e.value)
    v = condensed(dyadic(40, seed=2))
    v[5] = bad                                   # condensed (0, 6): lower entry (6, 0)
    with pytest.raises(RuntimeError) as e:
        engine.nj_dev(torch.as_tensor(v, device=DEV))
    assert "(6, 0)" in str(e.value)


def test_n_zero_is_an_argument_error():
    rc = _lib.lib().ppk_nj_dev(None, 0, 1, 0, 0, None, None, None)
    assert rc == 1 and b"n must be" in _lib.lib().ppk_last_error()


def test_two_calls_identical_bits():
    D = dyadic(900, seed=9, hi=5)          # heavy ties
    a = device_nj(D)
    b = device_nj(D)
    assert_same(a, b)


def test_generate_nj_tree_cuda_equals_host_path(synth_dist):
    n = 500
    sq = engine.long_to_square_dev(synth_dist, 0, 2000)[:n, :n].contiguous()
    labels = ["sample_%d" % i for i in range(n)]
    s_dev = trees.generate_nj_tree(sq, labels, "unused")
    join, lens = engine.nj(sq.cpu().numpy())
    assert s_dev == trees.nj_newick(join, lens, labels)
    assert s_dev == trees.generate_nj_tree(sq.cpu().numpy(), labels, "unused", rapidnj="ignored", threads=8)
