"""GPU tests of the lineages within every strain (ppk_strain_knn*, ppk_strain_ranks*, engine.strain_knn_dev /
strain_ranks_dev, poppunk_amd.lineages).  Everything is compared bit for bit with the numpy restatement
(tests/lineage_model.py, which goes strain by strain through oracle.prune_long / long_to_square / knn / lower_rank):
indices with array_equal, distances through their bit patterns; there are no tolerances.

The strain sizes 2, 3, 63, 64, 65, 256, 257 and 300 add up to 1 010 members, and a sample is in one strain at most, so
the matrix that holds them has 1 050 samples (40 in no strain), not "about 700"."""
import ctypes as C
import functools

import numpy as np
import pytest

import lineage_model as model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine  # noqa: E402

DEV = "cuda:0"
SIZES = [2, 3, 63, 64, 65, 256, 257, 300]       # 65: the longest wave-route strain; 66 .. 4 097: the LDS route
N_BIG = 1050


def make_strains(n, sizes, seed):
    """Strains that interleave in id space, each list shuffled; the samples left over are in no strain."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n).astype(np.int64)
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert seg_off[-1] < n
    return perm[:seg_off[-1]].copy(), seg_off


def make_dist(n, seed):
    """float32 [n(n-1)/2, 2]: column 0 with many duplicated values and zeros, column 1 nearly all distinct."""
    rng = np.random.default_rng(seed)
    rows = n * (n - 1) // 2
    d = rng.random((rows, 2)).astype(np.float32)
    d[:, 0] = np.floor(d[:, 0] * 64) / 64
    d[rng.integers(0, rows, rows // 50), 1] = 0.0
    return d


def as_dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def run_knn(dist, members, seg_off, depth, col=0):
    got = engine.strain_knn_dev(as_dev(dist, np.float32), as_dev(members, np.int64), seg_off, depth, col)
    return tuple(t.cpu().numpy() for t in got)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_lists(got, want, what=""):
    for g, w, name in zip(got[:2], want[:2], "ij"):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, name)
    assert got[2].dtype == np.float32 and np.array_equal(bits(got[2]), bits(want[2])), (what, "dist")


def cut(lists, seg_off, full, depth):
    """The lists at a smaller depth from the lists at depth `full`: the head of every row."""
    keep, at = [], 0
    for n_s in np.diff(seg_off):
        d_full, d_cut = min(full, n_s - 1), min(depth, n_s - 1)
        idx = at + (np.arange(n_s)[:, None] * d_full + np.arange(d_cut)[None, :]).ravel()
        keep.append(idx)
        at += n_s * d_full
    keep = np.concatenate(keep)
    return tuple(a[keep] for a in lists)


@functools.lru_cache(maxsize=None)
def big_case():
    members, seg_off = make_strains(N_BIG, SIZES, 5)
    dist = make_dist(N_BIG, 6)
    want = {col: model.strain_knn(dist, N_BIG, members, seg_off, N_BIG, col) for col in (0, 1)}
    return dist, members, seg_off, want


@pytest.mark.parametrize("col", [0, 1])
@pytest.mark.parametrize("depth", [1, 8, N_BIG])
def test_strain_sizes(col, depth):
    dist, members, seg_off, want = big_case()
    got = run_knn(dist, members, seg_off, depth, col)
    assert len(got[0]) == engine.strain_nnz(seg_off, depth)
    assert_lists(got, cut(want[col], seg_off, N_BIG, depth), "depth %d" % depth)


@pytest.mark.parametrize("options", [{"lineage_lds_keys": 128}, {"lineage_lds_keys": 128, "lineage_scratch_mb": 1},
                                     {"lineage_lds_keys": 64, "lineage_scratch_mb": 0}])
@pytest.mark.parametrize("depth", [8, N_BIG])
def test_routes(options, depth, ppk_option):
    """lineage_lds_keys 128 sends 256 / 257 / 300 through the long route (64: every strain past the wave route); one
    MiB of scratch cuts 256 and 300 into two bands each (255 and 299 keys of 16 bytes a row under 4/5 MiB: 205 and 175
    rows), none at all gives bands of one row."""
    dist, members, seg_off, want = big_case()
    default = run_knn(dist, members, seg_off, depth, 0)
    for name, value in options.items():
        ppk_option(name, value)
    got = run_knn(dist, members, seg_off, depth, 0)
    assert_lists(got, default, "against the default routing")
    assert_lists(got, cut(want[0], seg_off, N_BIG, depth), "against the model")


def tie_matrices(n):
    rng = np.random.default_rng(11)
    rows = n * (n - 1) // 2
    out = {"equal": np.full((rows, 2), 0.25, dtype=np.float32)}
    zeros = np.zeros((rows, 2), dtype=np.float32)
    zeros[rng.integers(0, rows, rows // 3)] = -0.0
    out["zeros"] = zeros
    # a tenth of the samples are copies of another sample: their rows of the square are equal
    sq = rng.random((n, n)).astype(np.float32)
    sq = np.triu(sq, 1) + np.triu(sq, 1).T
    for b in rng.permutation(n)[:n // 10]:
        a = (b + 1 + rng.integers(0, n - 1)) % n
        sq[b, :], sq[:, b] = sq[a, :], sq[:, a]
        sq[a, b] = sq[b, a] = 0.0
        sq[b, b] = 0.0
    iu = np.triu_indices(n, 1)
    out["copies"] = np.stack([sq[iu], sq[iu]], axis=1).astype(np.float32)
    tiny = (rng.integers(1, 5, (rows, 2)) * 2.0 ** -36).astype(np.float32)
    tiny[rng.integers(0, rows, rows // 4)] = rng.random((rows // 4, 2)).astype(np.float32)
    out["tiny"] = tiny
    return out


@pytest.mark.parametrize("name", ["equal", "zeros", "copies", "tiny"])
@pytest.mark.parametrize("lds_keys", [0, 64])
def test_ties(name, lds_keys, ppk_option):
    n = 200
    members, seg_off = make_strains(n, [2, 3, 30, 65, 70], 3)
    dist = tie_matrices(n)[name]
    ppk_option("lineage_lds_keys", lds_keys)
    got = run_knn(dist, members, seg_off, n, 0)
    assert_lists(got, model.strain_knn(dist, n, members, seg_off, n, 0), name)
    if name == "equal":
        at = 0
        for n_s in np.diff(seg_off):                         # column order: 0 .. n_s - 1 without the row itself
            j = got[1][at:at + n_s * (n_s - 1)].reshape(n_s, n_s - 1)
            want = np.asarray([[c for c in range(n_s) if c != r] for r in range(n_s)])
            assert np.array_equal(j, want)
            at += n_s * (n_s - 1)
    if name == "zeros":
        assert not np.signbit(got[2]).any()                  # -0.0 ties with 0.0 and comes back as 0.0


RANK_SIZES = [2, 3, 4, 6, 10, 65, 70]      # 2, 4 and 6: the smallest strains with n_s - 1 = the last rank of a list


@functools.lru_cache(maxsize=None)
def rank_case(name):
    n = 200
    members, seg_off = make_strains(n, RANK_SIZES, 17)
    dist = make_dist(n, 18) if name == "mixed" else tie_matrices(n)[name]
    lists = run_knn(dist, members, seg_off, n, 0)
    return seg_off, lists


@pytest.mark.parametrize("ranks", [[1], [1, 2, 3], [5]])
@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("epsilon", [1e-10, 0.05])
@pytest.mark.parametrize("name", ["mixed", "copies"])
def test_ranks(name, ranks, reciprocal, unique, epsilon):
    """0.05 is larger than the typical gap of a row of 64 or 69 uniform distances (1/64 steps in "mixed")."""
    seg_off, lists = rank_case(name)
    depth, m = 200, int(seg_off[-1])
    want_prefix, want_stream, want_numbers, _ = model.strain_ranks(lists, seg_off, depth, ranks, reciprocal, unique,
                                                                   epsilon)
    j_t, d_t = as_dev(lists[1], np.int64), as_dev(lists[2], np.float32)
    prefix, pi, pj, lv, sd = engine.strain_ranks_dev(j_t, d_t, seg_off, depth, ranks, reciprocal, unique, epsilon)
    assert np.array_equal(prefix.cpu().numpy(), want_prefix)
    a, b, level = pi.cpu().numpy(), pj.cpu().numpy(), lv.cpu().numpy()
    if reciprocal:
        assert (a < b).all()
    got = np.stack([np.minimum(a, b), np.maximum(a, b), level], axis=1)
    got = got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))]
    assert len(np.unique(got[:, :2], axis=0)) == len(got), "an unordered pair is in the stream twice"
    assert np.array_equal(got, want_stream)
    clusters, _ = engine.cluster_sweep_dev(pi, pj, lv, m, len(ranks)) if len(a) else (None, None)
    if clusters is None:
        clusters = torch.arange(m, 0, -1, dtype=torch.int32, device=DEV).repeat(len(ranks), 1)
    numbers = engine.strain_cluster_numbers(clusters, seg_off).cpu().numpy()
    assert np.array_equal(numbers, want_numbers)


def test_ranks_host_form_and_capacity():
    seg_off, lists = rank_case("mixed")
    m, nnz = int(seg_off[-1]), len(lists[1])
    ranks = np.asarray([1, 3], dtype=np.int32)
    want_prefix, want_stream, _, _ = model.strain_ranks(lists, seg_off, 200, [1, 3], True, False, 1e-10)
    prefix = np.zeros((2, m), dtype=np.int32)
    out = [np.zeros(nnz, dtype=np.int64) for _ in range(3)]
    sd = np.zeros(nnz, dtype=np.float32)
    llp, ip, fp = C.POINTER(C.c_longlong), C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(cap):
        n_out = C.c_size_t(0)
        rc = _lib.lib().ppk_strain_ranks(lists[1].ctypes.data_as(llp), lists[2].ctypes.data_as(fp),
                                         seg_off.ctypes.data_as(llp), len(seg_off) - 1, 200, ranks.ctypes.data_as(ip), 2,
                                         1, 0, 1e-10, 0, prefix.ctypes.data_as(ip), out[0].ctypes.data_as(llp),
                                         out[1].ctypes.data_as(llp), out[2].ctypes.data_as(llp), sd.ctypes.data_as(fp),
                                         cap, C.byref(n_out))
        return rc, int(n_out.value)
    assert call(1) == (_lib.ERR_CAPACITY, len(want_stream))
    assert call(nnz) == (_lib.OK, len(want_stream))
    k = len(want_stream)
    assert np.array_equal(prefix, want_prefix)
    assert np.array_equal(np.stack([a[:k] for a in out], axis=1)[np.lexsort((out[1][:k], out[0][:k]))], want_stream)


def test_knn_host_form():
    n = 200
    members, seg_off = make_strains(n, [2, 3, 30, 65, 70], 3)
    dist = make_dist(n, 4)
    nnz = engine.strain_nnz(seg_off, 8)
    oi, oj, od = np.zeros(nnz, dtype=np.int64), np.zeros(nnz, dtype=np.int64), np.zeros(nnz, dtype=np.float32)
    llp, fp = C.POINTER(C.c_longlong), C.POINTER(C.c_float)
    rc = _lib.lib().ppk_strain_knn(dist.ctypes.data_as(fp), n, 1, members.ctypes.data_as(llp),
                                   seg_off.ctypes.data_as(llp), len(seg_off) - 1, 8, 0, oi.ctypes.data_as(llp),
                                   oj.ctypes.data_as(llp), od.ctypes.data_as(fp))
    _lib.check(rc, "ppk_strain_knn")
    assert_lists((oi, oj, od), model.strain_knn(dist, n, members, seg_off, 8, 1))


def test_errors_name_the_first_offender():
    n = 100
    members, seg_off = make_strains(n, [5, 6, 7], 9)
    dist = make_dist(n, 10)
    bad = members.copy()
    bad[7], bad[12] = n, -1                                  # strain 1, member 2 comes first
    with pytest.raises(RuntimeError, match=r"ppk_strain_knn: strain 1, member 2: sample 100 outside \[0, 100\)"):
        run_knn(dist, bad, seg_off, 3)
    twice = members.copy()
    twice[13] = members[3]                                   # strain 2, member 2 repeats strain 0, member 3
    twice[16] = members[4]
    with pytest.raises(RuntimeError, match="ppk_strain_knn: strain 2, member 2: sample %d is already member 3 of "
                                           "strain 0" % members[3]):
        run_knn(dist, twice, seg_off, 3)
    one = np.asarray([0, 5, 6, 18], dtype=np.int64)
    with pytest.raises(RuntimeError, match="ppk_strain_knn: strain 1 has 1 members: a strain needs at least 2"):
        run_knn(dist, members, one, 3)
    assert_lists(run_knn(dist, members, seg_off, 3), model.strain_knn(dist, n, members, seg_off, 3))


def local_long(dist, n, mem):
    """The strain's long-form matrix in LOCAL order: row (a < b) is the matrix's row of (mem[a], mem[b])."""
    a, b = np.triu_indices(len(mem), 1)
    lo, hi = np.minimum(mem[a], mem[b]), np.maximum(mem[a], mem[b])
    return np.ascontiguousarray(dist[lo * (2 * n - lo - 1) // 2 + (hi - lo - 1)])


def same_coo(got, want, what):
    assert got.shape == want.shape, what
    for name in ("row", "col"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)
    assert got.data.dtype == want.data.dtype and np.array_equal(bits(got.data), bits(want.data)), (what, "data")


@pytest.mark.parametrize("flags", [dict(), dict(reciprocal_only=True, count_unique_distances=True, use_accessory=True,
                                                max_search_depth=8, ranks=[1, 2, 5])])
def test_fit_strain_lineages_equals_the_single_strain_fit(flags):
    """Per strain, array for array, what models.LineageRanks.fit (longToSquare -> get_kNN_distances -> lowerRank per
    rank, one strain at a time) gives on the strain's own long-form matrix."""
    from poppunk_amd import lineages, models
    n = 200
    sizes = [9, 10, 30, 66, 70]                       # 9: below min_count
    members, seg_off = make_strains(n, sizes, 23)
    dist = make_dist(n, 24)
    names = ["s%03d" % k for k in range(n)]
    strain_of = {"strain%d" % s: [names[g] for g in members[seg_off[s]:seg_off[s + 1]]] for s in range(len(sizes))}
    flags = dict(flags)
    ranks = flags.pop("ranks", [1, 2, 3])
    fitted = lineages.fit_strain_lineages(as_dev(dist, np.float32), names, strain_of, ranks, min_count=10, **flags)
    assert list(fitted) == ["strain1", "strain2", "strain3", "strain4"]
    for s in range(1, len(sizes)):
        mem = members[seg_off[s]:seg_off[s + 1]]
        single = models.LineageRanks(ranks, flags.get("max_search_depth", 10000), flags.get("reciprocal_only", False),
                                     flags.get("count_unique_distances", False),
                                     dist_col=1 if flags.get("use_accessory") else 0)
        single.fit(local_long(dist, n, mem))
        got, clusters, overall = fitted["strain%d" % s]
        same_coo(got.nn_dists, single.nn_dists, "nn_dists of strain %d" % s)
        for rank in ranks:
            same_coo(got.lower_rank_dists[rank], single.lower_rank_dists[rank], "rank %d of strain %d" % (rank, s))
            edges = np.stack([single.lower_rank_dists[rank].row, single.lower_rank_dists[rank].col], axis=1)
            want = model.print_clusters_numbers(model.components(len(mem), edges))
            assert [clusters[rank][names[g]] for g in mem] == want.tolist()
        assert list(overall) == ["Rank_%d" % r for r in ranks] + ["overall"]


@pytest.mark.parametrize("run", ["default", "flags"])
def test_golden_case_end_to_end(run, tmp_path, capsys):
    """python -m poppunk_amd.lineages --create-db on the golden case: the reference's files (lineage_golden.py says
    how the combined CSV's hash-ordered rows are compared)."""
    import lineage_golden
    lineage_golden.run_and_check(tmp_path, run, capsys)


def test_ranks_refuse_lists_that_are_not_a_strains():
    seg_off, lists = rank_case("mixed")
    j = lists[1].copy()
    at = int(engine.strain_nnz(seg_off[:5], 200))            # the first entry of strain 4 (10 members), row 0
    for value, what in ((10, "outside"), (0, "the row itself")):
        j[at] = value
        with pytest.raises(RuntimeError, match=r"ppk_strain_ranks: strain 4, member 0: a column outside \[0, 10\) or "
                                               "the row itself"):
            engine.strain_ranks_dev(as_dev(j, np.int64), as_dev(lists[2], np.float32), seg_off, 200, [1, 2])
