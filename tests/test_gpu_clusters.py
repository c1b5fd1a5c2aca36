"""GPU tests of the cluster numbers and pair sums (ppk_cluster_sweep*, ppk_cluster_pair_sums*):
every element against scipy's components ranked as printClusters ranks them / against a numpy accumulation of the
same fixed-point values, the argument errors by message, and multi_refine, iterate_clusters, RefineBoundary.fit(
multi_boundary=...) and printClusters end to end against the reference-derived fixture (tests/golden/clusters.npz,
clusters_csv.json)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, iterate, models, network, refine  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


# ---- cluster numbers ------------------------------------------------------------------------------------------------
def numbers_of_graph(i, j, n):
    """printClusters' ranking restated: components in the order of their smallest vertex (scipy's numbering), ranked by
    len - rankdata(sizes, 'ordinal'): size descending, equal sizes by component index descending; 1-based."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.stats import rankdata
    g = coo_matrix((np.ones(i.size, dtype=np.int8), (i, j)), shape=(n, n))
    k, labels = connected_components(g, directed=False)
    first = np.full(k, n)
    np.minimum.at(first, labels, np.arange(n))
    assert np.all(np.diff(first) > 0)                   # scipy numbers by smallest vertex
    sizes = np.bincount(labels, minlength=k)
    ranks = k - rankdata(sizes, method="ordinal").astype(np.int64)
    return (ranks[labels] + 1).astype(np.int32), k


def sweep_reference(i, j, o, n, n_off):
    out = np.zeros((n_off, n), dtype=np.int32)
    counts = np.zeros(n_off, dtype=np.int32)
    for t in range(n_off):
        if t and not (o == t).any():
            out[t], counts[t] = out[t - 1], counts[t - 1]
            continue
        sel = o <= t
        out[t], counts[t] = numbers_of_graph(i[sel], j[sel], n)
    return out, counts


def planted(n, n_off, empty, seed):
    """clusters of repeated sizes (many ties), each a random tree plus a few extra edges, its edges spread over the
    offsets that are not in `empty`; both orientations; shuffled"""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n - 40:                          # the last 40 or so vertices stay singletons
        sizes.append(int(rng.choice([2, 2, 3, 3, 5, 5, 8, 8, 21, 21, 64, 130])))
    sizes = [s for s in sizes if s > 0]
    while sum(sizes) > n - 40:
        sizes.pop()
    perm = rng.permutation(n)
    used = np.array([t for t in range(n_off) if t not in empty], dtype=np.int64)
    ei, ej = [], []
    at = 0
    for s in sizes:
        v = perm[at:at + s]
        at += s
        for k in range(1, s):
            ei.append(v[k])
            ej.append(v[rng.integers(0, k)])
        for _ in range(s // 4):
            a, b = rng.choice(s, 2, replace=False)
            ei.append(v[a])
            ej.append(v[b])
    e = np.unique(np.sort(np.stack([ei, ej], axis=1), axis=1), axis=0)
    i, j = e[:, 0].copy(), e[:, 1].copy()
    swap = rng.random(i.size) < 0.5
    i, j = np.where(swap, j, i), np.where(swap, i, j)
    o = rng.choice(used, size=i.size)
    order = rng.permutation(i.size)
    return i[order].astype(np.int64), j[order].astype(np.int64), o[order].astype(np.int64)


def run_dev(i, j, o, n, n_off, stride=1):
    if stride == 2:
        e = dev(np.stack([i, j], axis=1))
        i_t, j_t = e[:, 0], e[:, 1]
    else:
        i_t, j_t = dev(i), dev(j)
    c, k = engine.cluster_sweep_dev(i_t, j_t, None if o is None else dev(o), n, n_off)
    return c.cpu().numpy(), k.cpu().numpy()


@pytest.mark.parametrize("n", [1, 5])
def test_no_edges_is_all_singletons_under_the_tie_rule(n):
    z = np.zeros(0, dtype=np.int64)
    for n_off, o in ((1, None), (3, z)):
        c, k = run_dev(z, z, o, n, n_off)
        assert c.shape == (n_off, n) and np.array_equal(c, np.tile(n - np.arange(n), (n_off, 1)))
        assert np.array_equal(k, np.full(n_off, n))
        ch, kh = network.cluster_sweep(z, z, o, n, n_off)
        assert np.array_equal(ch, c) and np.array_equal(kh, k)


def test_equal_sizes_rank_by_component_index_descending():
    # n = 7: {0, 3, 4} and {1, 2, 6} have equal size, 5 is alone.  The component of the higher smallest vertex
    # ({1, 2, 6}) gets number 1.
    i = np.array([0, 4, 2, 6], dtype=np.int64)
    j = np.array([3, 3, 1, 1], dtype=np.int64)
    c, k = run_dev(i, j, None, 7, 1)
    assert c[0].tolist() == [2, 1, 1, 2, 2, 3, 1] and k.tolist() == [3]
    want, kk = numbers_of_graph(i, j, 7)
    assert np.array_equal(c[0], want) and kk == 3


@pytest.fixture(scope="module")
def planted_cases():
    n = 1500
    cases = {}
    for name, n_off, empty in (("one", 1, ()), ("forty", 40, (0, 17, 39)), ("max", 1023, ())):
        i, j, o = planted(n, n_off, set(empty), 11 + n_off)
        cases[name] = (i, j, o, n, n_off, sweep_reference(i, j, o, n, n_off))
    return cases


@pytest.mark.parametrize("name", ["one", "forty", "max"])
def test_planted_clusters_every_element(planted_cases, name):
    i, j, o, n, n_off, (want, want_k) = planted_cases[name]
    assert (i > j).any() and (i < j).any()
    sizes = np.bincount(np.bincount(want[-1])[1:])
    assert (sizes[1:] > 1).sum() >= 4                   # several sizes occur more than once: the tie rule decides
    c, k = run_dev(i, j, None if name == "one" else o, n, n_off)
    assert np.array_equal(k, want_k)
    assert np.array_equal(c, want)
    if name == "forty":
        assert np.array_equal(c[0], n - np.arange(n)) and np.array_equal(c[17], c[16]) and np.array_equal(c[39], c[38])
    # the [m, 2] edge list read in place, the host-array call, and a second call: the same bits
    c2, k2 = run_dev(i, j, None if name == "one" else o, n, n_off, stride=2)
    assert np.array_equal(c2, c) and np.array_equal(k2, k)
    if name != "max":
        ch, kh = network.cluster_sweep(i, j, None if name == "one" else o, n, n_off)
        assert np.array_equal(ch, c) and np.array_equal(kh, k)
    c3, k3 = run_dev(i, j, None if name == "one" else o, n, n_off)
    assert np.array_equal(c3, c) and np.array_equal(k3, k)


def test_reference_numbers_of_the_fixture_sweep():
    """growNetwork(write_clusters=...) of the reference on the `holes` triples: file k holds the numbers of the next
    graph that gains edges"""
    z = np.load(os.path.join(HERE, "golden", "clusters.npz"))
    net = np.load(os.path.join(HERE, "golden", "network_sweep.npz"))
    n, n_off = int(net["holes_n"]), int(net["holes_n_off"])
    c, k = run_dev(net["holes_i"], net["holes_j"], net["holes_idx"], n, n_off)
    assert np.array_equal(k, net["holes_stats"][:, 1])
    files = refine.boundary_files(z["holes_edge_counts"], k, n)
    assert [f for f, _ in files] == z["holes_file_idx"].tolist()
    assert np.array_equal(c[[idx for _, idx in files]], z["holes_numbers"])


def test_sweep_validation_errors_by_message():
    lib = _lib.lib()
    i, j, o = dev(np.array([0, 1, 2], dtype=np.int64)), dev(np.array([1, 2, 3], dtype=np.int64)), \
        dev(np.array([0, 1, 1], dtype=np.int64))
    out = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)

    def call(i_t, j_t, stride, o_t, m, n, n_off, out_t=out, cnt_t=cnt):
        rc = lib.ppk_cluster_sweep_dev(C.c_void_p(i_t.data_ptr()) if i_t is not None else None,
                                       C.c_void_p(j_t.data_ptr()) if j_t is not None else None, stride,
                                       C.c_void_p(o_t.data_ptr()) if o_t is not None else None, m, n, n_off,
                                       C.c_void_p(out_t.data_ptr()) if out_t is not None else None,
                                       C.c_void_p(cnt_t.data_ptr()) if cnt_t is not None else None, None)
        return rc, _lib.last_error()

    for args, msg in (((i, j, 1, o, 3, 4, 0), "ppk_cluster_sweep: n_off must be 1 .. 1023"),
                      ((i, j, 1, o, 3, 4, 1024), "ppk_cluster_sweep: n_off must be 1 .. 1023"),
                      ((i, j, 1, None, 3, 4, 2), "ppk_cluster_sweep: no offset array needs n_off == 1"),
                      ((i, j, 3, o, 3, 4, 2), "ppk_cluster_sweep: stride must be 1 or 2"),
                      ((None, None, 1, None, 0, 1 << 31, 1), "ppk_cluster_sweep: n_vertices must be < 2^31"),
                      ((i, j, 1, o, 1 << 31, 4, 2), "ppk_cluster_sweep: n_edges must be < 2^31"),
                      ((None, j, 1, o, 3, 4, 2), "ppk_cluster_sweep: NULL array"),
                      ((i, j, 1, o, 3, 4, 2, None), "ppk_cluster_sweep: NULL array"),
                      ((i, j, 1, o, 3, 4, 2, out, None), "ppk_cluster_sweep: NULL array")):
        rc, err = call(*args)
        assert rc == _lib.ERR_ARG and err == msg, (args[2:], err)
    rc, err = call(i, j, 1, o, 3, 3, 2)
    assert rc == _lib.ERR_ARG and err == "ppk_cluster_sweep: edge 2 (i=2, j=3, offset 1): vertex id out of range [0, 3)"
    loop = dev(np.array([1, 2, 2], dtype=np.int64))
    rc, err = call(i, loop, 1, o, 3, 4, 2)
    assert rc == _lib.ERR_ARG and err == "ppk_cluster_sweep: edge 2 (i=2, j=2, offset 1): self-loop"
    rc, err = call(i, j, 1, o, 3, 4, 1)
    assert rc == _lib.ERR_ARG and err == "ppk_cluster_sweep: edge 1 (i=1, j=2, offset 1): offset index out of range [0, 1)"
    with pytest.raises(RuntimeError, match="self-loop"):
        network.cluster_sweep([0, 2], [1, 2], [0, 0], 4, 1)
    # and the call still works afterwards
    c, k = run_dev(np.array([0], dtype=np.int64), np.array([1], dtype=np.int64), None, 3, 1)
    assert c.tolist() == [[1, 1, 2]] and k.tolist() == [2]


# ---- pair sums -------------------------------------------------------------------------------------------------------
def pair_reference(x, levels, shift):
    """every row quantised as specified, in int64, added to the bucket of the first level at which its pair meets"""
    n_levels, n = levels.shape
    ii, jj = np.triu_indices(n, 1)                     # the condensed order
    q = np.rint(x.astype(np.float64) * 2.0**shift).astype(np.int64)
    same = levels[:, ii] == levels[:, jj]
    meets = same.any(axis=0)
    t = np.argmax(same, axis=0)[meets]
    c = levels[t, ii[meets]]
    s = np.zeros((n_levels, n + 1), dtype=np.int64)
    k = np.zeros((n_levels, n + 1), dtype=np.int64)
    np.add.at(s, (t, c), q[meets])
    np.add.at(k, (t, c), 1)
    return s, k


def nested_levels(n, n_levels, seed, groups=120):
    """a random partition into `groups` clusters of mixed sizes, coarsened by merging ids pairwise every sixth level
    (so consecutive levels repeat); members interleaved over the vertex order"""
    rng = np.random.default_rng(seed)
    g = np.minimum((rng.random(n) ** 2 * groups).astype(np.int64), groups - 1)
    rows = []
    for t in range(n_levels):
        coarse = g >> (t // 6 if n_levels > 2 else t)
        rows.append(np.unique(coarse, return_inverse=True)[1].reshape(-1) + 1)
    return np.stack(rows).astype(np.int32)


def values(n_rows, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n_rows, 2), dtype=np.float32)
    x[rng.integers(0, n_rows, max(1, n_rows // 50))] = 0.0
    x[rng.integers(0, n_rows, max(1, n_rows // 50))] = 1.0
    x[0] = (1.0, 0.0)
    return x


def sweep_levels(n, n_off, seed):
    rng = np.random.default_rng(seed)
    ii, jj = np.triu_indices(n, 1)
    keep = rng.random(ii.size) < 1.2 / n
    o = rng.integers(0, n_off, int(keep.sum()))
    c, _ = network.cluster_sweep(ii[keep], jj[keep], o, n, n_off)
    return c


def level_configs(n):
    out = {"one_cluster": np.ones((1, n), dtype=np.int32),
           "singletons": np.arange(1, n + 1, dtype=np.int32).reshape(1, n),
           "mixed_1": nested_levels(n, 1, 3), "mixed_2": nested_levels(n, 2, 4), "mixed_40": nested_levels(n, 40, 5)}
    if n > 2:
        out["from_sweep"] = sweep_levels(n, 40, 6)
    else:                                                # two vertices, one edge at offset 3 of 5
        out["from_sweep"] = network.cluster_sweep([1], [0], [3], 2, 5)[0]
    return out


def run_pairs(x_t, levels, col, shift):
    s, k, used = engine.cluster_pair_sums_dev(x_t, dev(levels), col=col, shift=shift)
    assert used == shift
    return s.cpu().numpy(), k.cpu().numpy()


@pytest.mark.parametrize("n", [2, 65, 363])
def test_pair_sums_equal_numpy(n):
    n_rows = n * (n - 1) // 2
    x = values(n_rows, n)
    assert (x == 0).any() and (x == 1).any()
    x_t = dev(x)
    for name, levels in level_configs(n).items():
        iterate.check_nested(levels)
        for col, shift in ((0, 40), (1, 40), (0, 10)):
            want_s, want_k = pair_reference(x[:, col], levels, shift)
            s, k = run_pairs(x_t, levels, col, shift)
            assert np.array_equal(k, want_k), (name, col, shift)
            assert np.array_equal(s, want_s), (name, col, shift)
            if name == "singletons":
                assert not s.any() and not k.any()
            # the total count of every cluster, sub-clusters included, is |C| (|C| - 1) / 2
            _, tot_k = iterate.cluster_totals(levels, s, k)
            for t in range(levels.shape[0]):
                size = np.bincount(levels[t], minlength=n + 1)
                assert np.array_equal(tot_k[t], size * (size - 1) // 2)
        s2, k2 = run_pairs(x_t, levels, 0, 10)          # a second call: the same bits
        assert np.array_equal(s2, s) and np.array_equal(k2, k)
        sh, kh = np.zeros_like(s), np.zeros_like(k)       # the host-array call
        llp = C.POINTER(C.c_longlong)
        lv = np.ascontiguousarray(levels)
        _lib.check(_lib.lib().ppk_cluster_pair_sums(x.ctypes.data_as(C.POINTER(C.c_float)), n_rows, 0,
                                                    lv.ctypes.data_as(C.POINTER(C.c_int32)), lv.shape[0], 10, 0,
                                                    sh.ctypes.data_as(llp), kh.ctypes.data_as(llp)))
        assert np.array_equal(sh, s) and np.array_equal(kh, k)


def test_means_within_the_fixed_point_bound():
    """|device mean - exact mean of the float32 values| <= 2^-(shift + 1), checked in integers: a float32 in [0, 1] is a
    multiple of 2^-149, so S_exact = sum x 2^149 is an integer, and the claim is
    |S_dev 2^(149 - shift) - S_exact| <= cnt 2^(148 - shift).  cluster_means divides two exact integers, one float64
    rounding of a value <= 1 (at most 2^-54); it is held against the exact mean, a Fraction."""
    from fractions import Fraction
    n = 363
    x = values(n * (n - 1) // 2, 9)
    levels = nested_levels(n, 40, 5)
    ii, jj = np.triu_indices(n, 1)
    exact = [int(v) for v in (x[:, 0].astype(np.float64) * 2.0**149)]
    for shift in (40, 10):
        s, k = run_pairs(dev(x), levels, 0, shift)
        tot_s, tot_k = iterate.cluster_totals(levels, s, k)
        means = iterate.cluster_means(levels, s, k, shift)
        checked = 0
        for t in (0, 7, 20, 39):
            for c in np.unique(levels[t]):
                rows = np.flatnonzero((levels[t, ii] == c) & (levels[t, jj] == c))
                if rows.size == 0:
                    assert np.isnan(means[t, c])
                    continue
                s_exact = sum(exact[r] for r in rows)
                cnt = int(tot_k[t, c])
                assert cnt == rows.size
                assert abs(int(tot_s[t, c]) * 2**(149 - shift) - s_exact) <= cnt * 2**(148 - shift)
                exact_mean = Fraction(s_exact, cnt * 2**149)
                assert abs(Fraction(float(means[t, c])) - exact_mean) <= Fraction(1, 2**(shift + 1)) + Fraction(1, 2**54)
                checked += 1
        assert checked > 50


def test_pair_sum_argument_errors_by_message():
    lib = _lib.lib()
    n = 5
    x = np.full((10, 2), 0.5, dtype=np.float32)
    levels = dev(np.ones((2, n), dtype=np.int32))
    out = torch.zeros((2, 2, n + 1), dtype=torch.int64, device=DEV)

    def call(x_np, n_rows=10, col=0, lv=levels, n_levels=2, shift=40):
        x_t = dev(x_np)
        rc = lib.ppk_cluster_pair_sums_dev(C.c_void_p(x_t.data_ptr()), n_rows, col, C.c_void_p(lv.data_ptr()),
                                           n_levels, shift, C.c_void_p(out[0].data_ptr()),
                                           C.c_void_p(out[1].data_ptr()), None)
        return rc, _lib.last_error()

    assert call(x)[0] == _lib.OK
    for bad, row in ((np.nan, 3), (-0.25, 7), (1.5, 0), (np.inf, 5)):
        y = x.copy()
        y[row, 0] = bad
        y[9, 0] = -1.0                                      # a later offender too: the FIRST is named
        rc, err = call(y)
        assert rc == _lib.ERR_ARG and err.startswith("ppk_cluster_pair_sums: row %d: value " % row), err
        assert err.endswith("is not a finite number in [0, 1]")
        assert call(y, col=1)[0] == _lib.OK                # the other column is clean
    rc, err = call(x, col=2)
    assert rc == _lib.ERR_ARG and err == "ppk_cluster_pair_sums: col must be 0 or 1"
    rc, err = call(x, n_rows=9)
    assert rc == _lib.ERR_ARG and err.startswith("ppk_cluster_pair_sums: row count is not n(n-1)/2")
    for shift in (-1, 41):
        rc, err = call(x, shift=shift)
        assert rc == _lib.ERR_ARG and err == "ppk_cluster_pair_sums: shift must be 0 .. 40"
    rc, err = call(x, n_levels=0)
    assert rc == _lib.ERR_ARG and err == "ppk_cluster_pair_sums: n_levels must be 1 .. 1023"
    for bad_number in (0, n + 1):
        lv = np.ones((2, n), dtype=np.int32)
        lv[1, 3] = bad_number
        rc, err = call(x, lv=dev(lv))
        assert rc == _lib.ERR_ARG and err == "ppk_cluster_pair_sums: level 1, vertex 3: cluster number %d outside [1, 5]" \
            % bad_number
    assert call(x)[0] == _lib.OK


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    z = dict(np.load(os.path.join(HERE, "golden", "clusters.npz")))
    net = np.load(os.path.join(HERE, "golden", "network_sweep.npz"))
    z["dist"] = net["sweep1d_dist"]
    z["names"] = ["s%d" % k for k in range(int(net["sweep1d_n"]))]
    return z


def read_files(prefix, names):
    base = os.path.join(prefix, os.path.basename(prefix))
    found = {}
    for f in os.listdir(prefix):
        k = int(f[len(os.path.basename(prefix)) + len("_boundary"):-len("_clusters.csv")])
        rows = [line.split(",") for line in open(os.path.join(prefix, f)).read().splitlines()]
        assert rows[0] == ["Taxon", "Cluster"] and f == "%s_boundary%d_clusters.csv" % (os.path.basename(base), k)
        found[k] = {name: int(c) for name, c in rows[1:]}
        assert sorted(found[k]) == sorted(names)
    return found


def test_multi_refine_writes_the_reference_files(fixture, tmp_path, capfd):
    prefix = str(tmp_path / "multi")
    for dist in (fixture["dist"], dev(fixture["dist"])):
        kept, idx = refine.multi_refine(dist, fixture["names"], fixture["multi_mean0"], fixture["multi_mean1"],
                                        np.array([1.0, 1.0]), float(fixture["multi_s_max"]),
                                        int(fixture["multi_n_points"]), prefix)
        assert idx == fixture["multi_file_idx"].tolist()
        assert kept.dtype == np.int32 and np.array_equal(kept, fixture["multi_numbers"])
    found = read_files(prefix, fixture["names"])
    assert sorted(found) == idx
    for k, row in zip(idx, fixture["multi_numbers"]):
        assert found[k] == dict(zip(fixture["names"], row.tolist()))
    assert "Search range (" in capfd.readouterr().err
    # the files are what iterate reads back
    assert np.array_equal(iterate.levels_of_files(os.path.join(prefix, "multi"), fixture["names"]),
                          fixture["multi_numbers"])


def test_iterate_gives_the_reference_family_and_means(fixture, tmp_path):
    names = fixture["names"]
    out = str(tmp_path / "it")
    res = iterate.iterate_clusters(fixture["multi_numbers"], names, dev(fixture["dist"]), cutoff=0.1, output=out)
    assert list(res["family"].keys()) == fixture["iter_ids"].tolist()
    for c, row in zip(fixture["iter_ids"].tolist(), fixture["iter_members"]):
        assert res["family"][c] == {names[v] for v in np.flatnonzero(row)}
    assert res["sorted"] == fixture["iter_sorted"].tolist()
    got = np.array([res["avg_pi"][c] for c in fixture["iter_ids"].tolist()])
    worst = np.abs(got - fixture["iter_avg_pi"]).max()
    print("Avg_Pi: max |device - reference| = %.3e, allowance %.3e" % (worst, float(fixture["iter_allowance"])))
    assert worst <= float(fixture["iter_allowance"])
    # a host matrix gives the same values to the bit
    res2 = iterate.iterate_clusters(fixture["multi_numbers"], names, fixture["dist"], cutoff=0.1)
    assert res2["avg_pi"] == res["avg_pi"] and res2["cut_clusters"] == res["cut_clusters"]
    lines = open(out + ".clusters.csv").read().splitlines()
    assert lines[0] == "Cluster,Avg_Pi,Taxa" and [int(x.split(",")[0]) for x in lines[1:]] == res["sorted"]
    assert open(out + ".tree.nwk").read() == res["newick"] and res["newick"].endswith(")root:0.00000;\n")
    cut = [line.split(",") for line in open(out + ".cutoff_clusters.csv").read().splitlines()]
    assert cut[0] == ["Isolate", "Cluster"] and {r[0] for r in cut[1:]} == set(names)
    with pytest.raises(ValueError, match="not nested"):
        iterate.iterate_clusters(fixture["multi_numbers"][::-1], names, fixture["dist"])


def test_fit_with_multi_boundary_writes_the_files_and_fits_the_same(fixture, tmp_path):
    start = tmp_path / "start.txt"
    start.write_text("start %r,%r\nend %r,%r\n" % (*fixture["multi_mean0"].tolist(), *fixture["multi_mean1"].tolist()))
    model = types.SimpleNamespace(scale=np.array([1.0, 1.0]))
    plain, multi = models.RefineBoundary(), models.RefineBoundary()
    y0 = plain.fit(fixture["dist"], fixture["names"], model, 0.0, 0.0, startFile=str(start))
    prefix = str(tmp_path / "fit")
    y1 = multi.fit(fixture["dist"], fixture["names"], model, 0.0, 0.0, startFile=str(start), multi_boundary=5,
                   outPrefix=prefix)
    assert np.array_equal(y0, y1)
    assert (plain.optimal_x, plain.optimal_y, plain.optimal_s) == (multi.optimal_x, multi.optimal_y, multi.optimal_s)
    kept, idx = multi.multi_boundary_clusters
    found = read_files(prefix, fixture["names"])
    assert 1 <= len(found) <= 5 and sorted(found) == idx and max(idx) <= 4
    for k, row in zip(idx, kept):
        assert found[k] == dict(zip(fixture["names"], row.tolist()))
    iterate.check_nested(kept)
    assert not hasattr(plain, "multi_boundary_clusters")


def test_print_clusters_on_a_cuda_edge_tensor():
    with open(os.path.join(HERE, "golden", "clusters_csv.json")) as f:
        case = {c["name"]: c for c in json.load(f)["naming"]}["no_old_file"]
    e = np.array(case["edges"], dtype=np.int64)
    for G in ((dev(e), case["n"]), (e, case["n"])):
        clustering, merged = network.printClusters(G, case["names"], printCSV=False)
        assert clustering == case["clustering"] and merged == []
        assert np.array_equal(network.cluster_numbers(G), np.array(case["numbers"]))
