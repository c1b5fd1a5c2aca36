"""Pair-list distances from resident sketches on a real MI355X (ppk_dist_pairs_dev).

The contract is bit equality with the dense kernel: "equals dense" below is torch.equal on an integer view against
engine.dist(...)[rows] for the same databases, k list, table and options.  The dense pass is the oracle DESIGN.md 3.1
names ("a pair's result does not depend on which kernel, tile, band or wavefront computed it"); the CPU oracle pins
the dense pass itself (tests/test_gpu_dist.py) and is compared once here as well."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from poppunk_amd import _lib, engine, models, pp_sketchlib, synth

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
TOL = 1e-6          # tests/test_gpu_dist.py's


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rows_of(pairs, n_ref, n_qry=0):
    """Dense rows of edge-form pairs (either orientation)."""
    a, b = np.minimum(pairs[:, 0], pairs[:, 1]), np.maximum(pairs[:, 0], pairs[:, 1])
    if n_qry:
        return (b - n_ref) * n_ref + a
    return a * n_ref - a * (a + 1) // 2 + (b - a - 1)


def _random_pairs(n, m, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n * (n - 1) // 2, size=m)
    pairs = engine.rows_to_pairs(rows, n)
    flip = rng.random(m) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    return rows, pairs


@pytest.fixture(scope="module")
def set300():
    """n = 300 (the sample axis is padded to 512), s64 = 16, the default k list: database, table, dense result."""
    sk, member = synth.make_sketches(300, KMERS, cluster_size=30)
    tbl = synth.random_match_table(KMERS)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dense, failed = engine.dist(db, None, KMERS, tbl)
    return {"sk": sk, "member": member, "tbl": tbl, "db": db, "dense": dense, "failed": int(failed.item())}


@pytest.fixture(scope="module")
def unrelated200():
    """Different-cluster pairs match by chance only: fewer than 2 usable k, rows (0, 0), counted."""
    sk, _ = synth.make_sketches(200, KMERS, cluster_size=20, related=False)
    tbl = synth.random_match_table(KMERS)
    want, n_failed = oracle.query(sk, None, KMERS, 16, 14, tbl, threads=4)
    zero = (want == 0).all(axis=1)
    # the fixture has failing and passing pairs, and (0, 0) marks exactly the failing ones
    assert 0 < n_failed < want.shape[0] and int(zero.sum()) == n_failed
    db = engine.SketchDB(sk, 16, 14, device=0)
    dense, failed = engine.dist(db, None, KMERS, tbl)
    assert int(failed.item()) == n_failed
    return {"tbl": tbl, "db": db, "dense": dense, "failed": n_failed, "zero": zero}


def test_shuffled_self_list_both_orientations(set300):
    n = 300
    rows = np.random.default_rng(1).permutation(n * (n - 1) // 2)
    pairs = engine.rows_to_pairs(rows, n)
    pairs[1::2] = pairs[1::2][:, ::-1]
    got, failed = engine.dist_pairs(set300["db"], None, KMERS, set300["tbl"], _t(pairs))
    assert _same(got, set300["dense"][_t(rows)])
    assert int(failed.item()) == set300["failed"]
    want, wf = oracle.query(set300["sk"], None, KMERS, 16, 14, set300["tbl"], threads=4)
    assert np.abs(got.cpu().numpy() - want[rows]).max() <= TOL and wf == set300["failed"]
    # the (i, j) pair of tensors is the same list
    again, _ = engine.dist_pairs(set300["db"], None, KMERS, set300["tbl"], (_t(pairs[:, 0]), _t(pairs[:, 1])))
    assert _same(again, got)


def test_duplicates_and_chunking(unrelated200, ppk_option):
    import torch
    u = unrelated200
    rows, pairs = _random_pairs(200, 10000, 2)
    assert np.unique(rows).size < rows.size
    want = u["dense"][_t(rows)]
    n_failed = int(u["zero"][rows].sum())          # occurrences, not distinct pairs
    assert n_failed > 0
    p_t = _t(pairs)
    for chunk in (0, 64, 1000, 4097):
        ppk_option("pairs_chunk", chunk)
        got, failed = engine.dist_pairs(u["db"], None, KMERS, u["tbl"], p_t)
        assert _same(got, want), chunk
        assert int(failed.item()) == n_failed, chunk
    ppk_option("pairs_chunk", 0)
    side = torch.cuda.Stream(device=0)
    side.wait_stream(torch.cuda.current_stream(0))
    with torch.cuda.stream(side):
        got, failed = engine.dist_pairs(u["db"], None, KMERS, u["tbl"], p_t)
    side.synchronize()
    assert _same(got, want) and int(failed.item()) == n_failed


def test_ref_query_ids(set300):
    n_ref, n_qry = 257, 43          # the ref axis padded to 512, the query axis to 256
    sk, tbl = set300["sk"], set300["tbl"]
    rdb, qdb = engine.SketchDB(sk[:n_ref], 16, 14), engine.SketchDB(sk[n_ref:], 16, 14)
    dense, df = engine.dist(rdb, qdb, KMERS, tbl)
    rows = np.random.default_rng(3).permutation(n_ref * n_qry)
    pairs = engine.rows_to_pairs(rows, n_ref, n_qry)
    assert np.array_equal(_rows_of(pairs, n_ref, n_qry), rows)
    want = dense[_t(rows)]
    for off in (0, 1000):
        for swap in (False, True):
            p = pairs[:, ::-1] if swap else pairs
            got, failed = engine.dist_pairs(rdb, qdb, KMERS, tbl, _t(p + off), int_offset=off)
            assert _same(got, want), (off, swap)
            assert int(failed.item()) == int(df.item())


def test_multi_cluster_random_table_pins_the_orientation(set300):
    sk, member = set300["sk"], set300["member"]
    n_clu = 3
    tbl = synth.random_match_table(KMERS, n_clu=n_clu)
    tbl = (tbl * np.random.Generator(np.random.PCG64(11)).uniform(0.5, 3.0, size=tbl.shape)).astype(np.float32)
    assert not np.array_equal(tbl, tbl.transpose(0, 2, 1))          # (ref, query) and (query, ref) differ
    clu = (member % n_clu).astype(np.uint16)
    db = engine.SketchDB(sk, 16, 14, clusters=clu)
    dense, _ = engine.dist(db, None, KMERS, tbl)
    rows, pairs = _random_pairs(300, 6000, 4)
    got, _ = engine.dist_pairs(db, None, KMERS, tbl, _t(pairs))
    assert _same(got, dense[_t(rows)])
    rdb, qdb = engine.SketchDB(sk[:200], 16, 14, clusters=clu[:200]), engine.SketchDB(sk[200:], 16, 14, clusters=clu[200:])
    dense, _ = engine.dist(rdb, qdb, KMERS, tbl)
    rows = np.random.default_rng(5).integers(0, 200 * 100, size=6000)
    got, _ = engine.dist_pairs(rdb, qdb, KMERS, tbl, _t(engine.rows_to_pairs(rows, 200, 100)))
    assert _same(got, dense[_t(rows)])


def test_failing_pairs(unrelated200):
    u = unrelated200
    n = 200
    rows = np.arange(n * (n - 1) // 2)
    got, failed = engine.dist_pairs(u["db"], None, KMERS, u["tbl"], _t(engine.rows_to_pairs(rows, n)))
    assert _same(got, u["dense"]) and int(failed.item()) == u["failed"]
    assert np.array_equal((got.cpu().numpy() == 0).all(axis=1), u["zero"])


def test_flags(set300):
    sk, tbl, db = set300["sk"], set300["tbl"], set300["db"]
    rows, pairs = _random_pairs(300, 3000, 6)
    p_t = _t(pairs)
    got, _ = engine.dist_pairs(db, None, KMERS, tbl, p_t, counts=True)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), oracle.match_counts(sk, None, 16, 14, threads=4)[rows])
    for rc in (True, False):
        dense, _ = engine.dist(db, None, KMERS, tbl, random_correct=rc, jaccard=True)
        got, _ = engine.dist_pairs(db, None, KMERS, tbl, p_t, random_correct=rc, jaccard=True)
        assert got.shape == (3000, 5) and _same(got, dense[_t(rows)]), rc
    # identical and disjoint sketches (test_identical_and_disjoint_sketches): 1024 / 0 / 0 matches at every k
    rng = np.random.Generator(np.random.PCG64(7))
    bins = rng.integers(0, 1 << 14, size=(3, 5, 1024), dtype=np.uint16)
    bins[1] = bins[0]
    bins[2] = (bins[0] + 1) & 0x3FFF
    three = synth.bitslice(bins, 14)
    got, _ = pp_sketchlib.query_pairs_arrays(three, None, KMERS, 16, 14, [[0, 1], [2, 0], [1, 2]], counts=True)
    assert np.array_equal(got, [[1024] * 5, [0] * 5, [0] * 5])
    d, failed = pp_sketchlib.query_pairs_arrays(three, None, KMERS, 16, 14, [[0, 1], [2, 0], [1, 2]],
                                                random_correct=False)
    assert failed == 2 and np.array_equal(d, np.zeros((3, 2)))


def _wide_table(kmers):
    return synth.random_match_table(kmers, genome_length=20_000 if min(kmers) < 10 else 2_000_000)


SHAPES = {
    # name: (n, k list, s64, bbits, options)
    "s64_156": (40, np.arange(13, 29, 3), 156, 14, {}),
    "s64_1": (70, KMERS, 1, 14, {}),
    "wide_k": (24, np.arange(6, 16), 156, 14, {}),
    "unfused_bbits13": (24, np.arange(6, 16), 156, 13, {}),
    "unfused_nk129": (24, np.arange(3, 3 + 129), 16, 14, {}),
    "collision_adjust": (40, KMERS, 256, 14, {"ext_collision_adjust": 1}),
    "fit_skip": (40, KMERS, 256, 14, {"ext_fit_skip": 1}),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shape_classes(shape, ppk_option):
    n, kmers, s64, bbits, options = SHAPES[shape]
    kmers = np.asarray(kmers, dtype=np.int32)
    for name, value in options.items():
        ppk_option(name, value)
    if shape == "collision_adjust":
        assert (64 * s64) >> bbits > 0
    sk, _ = synth.make_sketches(n, kmers, sketchsize64=s64, bbits=bbits, cluster_size=8, seed=n + s64)
    tbl = _wide_table(kmers)
    db = engine.SketchDB(sk, s64, bbits, device=0)
    rows, pairs = _random_pairs(n, 2000, 7)
    all_rows = np.arange(n * (n - 1) // 2)
    fitted = 0
    # with the table, and without the correction: under a 20 kb genome's table the lists from k = 6 lose their first
    # k to the floor and every fit fails, which checks the failure path only
    for rc in (True, False):
        dense, df = engine.dist(db, None, kmers, tbl, random_correct=rc)
        got, failed = engine.dist_pairs(db, None, kmers, tbl, _t(pairs), random_correct=rc)
        assert _same(got, dense[_t(rows)]), rc
        _, failed = engine.dist_pairs(db, None, kmers, tbl, _t(engine.rows_to_pairs(all_rows, n)), random_correct=rc)
        assert int(failed.item()) == int(df.item()), rc
        fitted += all_rows.size - int(df.item())
    assert fitted > 0


def _raw_call(db, qdb, tbl, pairs_t, out_t):
    k = np.ascontiguousarray(KMERS)
    t = np.ascontiguousarray(tbl, dtype=np.float32)
    return _lib.lib().ppk_dist_pairs_dev(db._h, qdb._h if qdb is not None else None, k.ctypes.data_as(C.POINTER(C.c_int32)),
                                         t.ctypes.data_as(C.POINTER(C.c_float)), 1, engine.FLAG_RANDOM_CORRECT,
                                         C.c_void_p(pairs_t.data_ptr()), C.c_void_p(pairs_t.data_ptr() + 8), 2,
                                         pairs_t.shape[0], 0, C.c_void_p(out_t.data_ptr()), None, None)


def test_errors_are_answered_before_a_sketch_is_read(set300):
    import torch
    db, tbl, sk = set300["db"], set300["tbl"], set300["sk"]
    good = engine.rows_to_pairs(np.arange(100), 300)
    for p, bad, what in ((17, (5, 300), "out of range"), (3, (-1, 7), "out of range"), (99, (12, 12), "itself")):
        pairs = good.copy()
        pairs[p] = bad
        with pytest.raises(RuntimeError, match=r"pair %d \(i=%d, j=%d\).*%s" % (p, bad[0], bad[1], what)):
            engine.dist_pairs(db, None, KMERS, tbl, _t(pairs))
        out = torch.full((100, 2), -7.0, dtype=torch.float32, device="cuda:0")
        assert _raw_call(db, None, tbl, _t(pairs), out) == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
    # the first offender is named
    pairs = good.copy()
    pairs[60] = (0, 300)
    pairs[40] = (7, 7)
    with pytest.raises(RuntimeError, match=r"pair 40 "):
        engine.dist_pairs(db, None, KMERS, tbl, _t(pairs))
    # ref x query: both ids on one side, and ids past the queries
    rdb, qdb = engine.SketchDB(sk[:257], 16, 14), engine.SketchDB(sk[257:], 16, 14)
    good = engine.rows_to_pairs(np.arange(100), 257, 43)
    for p, bad, what in ((8, (3, 200), "one side"), (9, (260, 270), "one side"), (10, (0, 300), "out of range")):
        pairs = good.copy()
        pairs[p] = bad
        with pytest.raises(RuntimeError, match=r"pair %d .*%s" % (p, what)):
            engine.dist_pairs(rdb, qdb, KMERS, tbl, _t(pairs))
        out = torch.full((100, 2), -7.0, dtype=torch.float32, device="cuda:0")
        assert _raw_call(rdb, qdb, tbl, _t(pairs), out) == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
    empty, failed = engine.dist_pairs(db, None, KMERS, tbl, torch.empty((0, 2), dtype=torch.int64, device="cuda:0"))
    assert empty.shape == (0, 2) and int(failed.item()) == 0


def test_edge_weights_without_a_matrix(set300):
    import torch
    db, tbl, dense = set300["db"], set300["tbl"], set300["dense"]
    x_max, y_max = synth.boundary_for_quantile(dense.cpu().numpy(), 0.08)
    edges, _ = engine.dist_edges(db, None, KMERS, tbl, slope=2, x_max=x_max, y_max=y_max)
    assert 1000 < edges.shape[0] < 10000
    for kind in ("core", "accessory", "euclidean"):
        want = engine.edge_weights_dev(dense, edges, kind)
        got = engine.edge_weights_from_sketches(db, None, KMERS, tbl, edges, kind)
        assert _same(got, want), kind
        tree_w, comp_w, _ = engine.mst_dev(edges, want, 300)
        tree_g, comp_g, _ = engine.mst_dev(edges, got, 300)
        assert comp_w == comp_g and torch.equal(tree_w, tree_g)


def test_bgmm_fit_without_a_matrix(set300):
    import torch
    db, tbl, dense = set300["db"], set300["tbl"], set300["dense"]
    rows = models.sample_rows(44850, 5000, 42)
    want = models.BGMMModel.fit_dev(dense[_t(rows)].contiguous(), 2, max_samples=None, seed=42, assign_points=False)
    for kw in ({"rows": rows}, {}):          # the draw of fit_from_sketches is sample_rows'
        got = models.BGMMModel.fit_from_sketches(db, KMERS, tbl, max_components=2, max_samples=5000, seed=42, **kw)
        for name in ("weights", "means", "covariances", "scale"):
            a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
        assert got.within_label == want.within_label
        assert torch.equal(got.labels, want.labels) and got.labels.shape[0] == 5000
        assert got.fit_info["n_iter"] == want.fit_info["n_iter"]


def test_dbscan_fit_without_a_matrix():
    # (the population of tests/test_gpu_dbscan.py's fit test: two clusters of distances that DBSCAN tells apart)
    sk, _ = synth.make_sketches(300, KMERS, cluster_size=60)
    tbl = synth.random_match_table(KMERS)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dense, _ = engine.dist(db, None, KMERS, tbl)
    rows = models.sample_rows(44850, 2000, 42)
    want = models.DBSCANModel()
    want.fit_dev(dense[_t(rows)].contiguous(), 10, 0.01, max_samples=None, seed=42, assign_points=False)
    got = models.DBSCANModel()
    got.fit_from_sketches(db, KMERS, tbl, 10, 0.01, max_samples=2000, seed=42)
    assert np.asarray(got.scale).tobytes() == np.asarray(want.scale).tobytes()
    assert got.within_label == want.within_label and got.n_clusters == want.n_clusters
    assert np.array_equal(got.subsample_labels, want.subsample_labels) and got.subsample_labels.shape[0] == 2000
