"""GPU tests of query assignment (ppk_query_links*, ppk_cluster_extend*): every element against the
numpy restatement of tests/test_assign_host.py and, for the numbers, against cluster_numbers_dev on the explicit full
graph; the argument errors by message; every case of the reference-derived fixture (tests/golden/assign.json) end to
end on the device; assign_from_sketches against distances -> model.assign -> the mirrors.  Everything is exact."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import assign, engine, models, network, synth  # noqa: E402
from test_assign_host import (CASES, DOC, N_REF, arrays, check_golden_case, extend_restated, links_restated,  # noqa: E402
                              ranking_restated, run_golden_case)

DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


# ---- links -----------------------------------------------------------------------------------------------------------
N_REF_L, N_QRY_L = 700, 193


def links_input():
    """(labels, ordered [m, 2], shuffled-and-mixed [m', 2]): about 150 components of labels that are neither dense nor
    ordered; query 0 of degree 1, query 1 of degree 0, query 2 linked to all 700 references (a dozen wave iterations,
    more distinct labels than the LDS set holds), query 3 to references of 130 components (one over the set's 128),
    query 4 to 128 exactly, the last query to five; the rest at random, some with repeated edges"""
    rng = np.random.default_rng(11)
    comp = rng.integers(0, 150, N_REF_L)
    comp[:150] = np.arange(150)                            # every component exists
    rng.shuffle(comp)
    names = rng.permutation(N_REF_L)[:150]                 # the label VALUES: any numbers in [0, n_ref)
    label = names[comp].astype(np.int32)
    one_of = [np.flatnonzero(comp == c) for c in range(150)]
    rows = {0: [5], 1: [], 2: list(range(N_REF_L)),
            3: [int(one_of[c][0]) for c in range(130)] + [int(one_of[c][-1]) for c in range(40)],
            4: [int(r) for c in range(128) for r in one_of[c][:2]],
            N_QRY_L - 1: [int(one_of[c][0]) for c in (7, 7, 3, 149, 0, 64)]}
    for q in range(5, N_QRY_L - 1):
        k = int(rng.integers(0, 40))
        rows[q] = rng.integers(0, N_REF_L, k).tolist() if q % 7 else sorted(rng.integers(0, N_REF_L, k).tolist())
    ordered = np.array([(r, N_REF_L + q) for q in range(N_QRY_L) for r in rows[q]], dtype=np.int64)
    # shuffled, orientation mixed, with query-query and reference-reference edges in between
    extra = np.concatenate([np.stack([rng.integers(0, N_REF_L, 300), rng.integers(0, N_REF_L, 300)], axis=1),
                            N_REF_L + np.stack([rng.integers(0, N_QRY_L, 200), rng.integers(0, N_QRY_L, 200)], axis=1)])
    extra = extra[extra[:, 0] != extra[:, 1]]
    mixed = np.concatenate([ordered, extra])
    flip = rng.random(mixed.shape[0]) < 0.5
    mixed[flip] = mixed[flip][:, ::-1]
    mixed = mixed[rng.permutation(mixed.shape[0])]
    return label, ordered, mixed


LINKS = links_input()


def got_links(edges, label, n_qry, max_links):
    return tuple(t.cpu().numpy() for t in engine.query_links_dev(dev(edges), dev(label), n_qry, max_links))


@pytest.mark.parametrize("max_links", [1, 4, 64])
def test_links_match_the_restatement_in_row_order_and_shuffled(max_links):
    label, ordered, mixed = LINKS
    want = links_restated(ordered[:, 0], ordered[:, 1], label, N_QRY_L, max_links)
    assert want[0][:4].tolist() == [1, 0, 700, 170] and want[0][4] > 128 and want[1][:5].tolist() == [1, 0, 150, 130, 128]
    assert want[1][-1] == 5 and want[0][-1] == 6
    a = got_links(ordered, label, N_QRY_L, max_links)
    b = got_links(mixed, label, N_QRY_L, max_links)
    for k in range(3):
        assert a[k].dtype == np.int32 and np.array_equal(a[k], want[k]), k
        assert a[k].tobytes() == b[k].tobytes(), k           # the sort route: the same bits
    # the ordered stream followed by skipped edges is still ordered (the stream cluster_extend takes)
    tail = np.array([(0, 1), (N_REF_L, N_REF_L + 1)], dtype=np.int64)
    c = got_links(np.concatenate([ordered, tail]), label, N_QRY_L, max_links)
    assert all(np.array_equal(c[k], want[k]) for k in range(3))


def test_links_of_separate_arrays_and_of_the_host_twin():
    label, ordered, mixed = LINKS
    want = links_restated(ordered[:, 0], ordered[:, 1], label, N_QRY_L, 8)
    i_t, j_t = dev(mixed[:, 1].copy()), dev(mixed[:, 0].copy())
    got = engine.query_links_dev((i_t, j_t), dev(label), N_QRY_L, 8)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    for e in (ordered, mixed):
        got = network.query_links(e[:, 0], e[:, 1], label, N_QRY_L, 8)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_links_without_edges_and_of_one_query():
    label = LINKS[0]
    none = np.zeros((0, 2), dtype=np.int64)
    degree, n_links, links = got_links(none, label, 5, 4)
    assert degree.tolist() == [0] * 5 and n_links.tolist() == [0] * 5 and (links == -1).all() and links.shape == (5, 4)
    e = np.array([(3, N_REF_L), (N_REF_L, 9), (3, N_REF_L)], dtype=np.int64)
    for edges in (e, e[::-1].copy()):
        got = got_links(edges, label, 1, 4)
        want = links_restated(e[:, 0], e[:, 1], label, 1, 4)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert got_links(np.array([(0, 1)], dtype=np.int64), label, 0, 4)[0].shape == (0,)


# ---- extend ----------------------------------------------------------------------------------------------------------
N_REF_E, N_QRY_E = 1000, 257


def extend_input():
    """a reference network of planted clusters of repeated sizes (random trees plus extra edges) and about 40
    singletons; 257 queries: unlinked, singly linked, merging two and three components, query-query chains that merge
    components, clusters made only of queries"""
    rng = np.random.default_rng(5)
    sizes = []
    while sum(sizes) < N_REF_E - 40:
        sizes.append(int(rng.choice([2, 2, 3, 3, 5, 5, 8, 8, 21, 21, 64, 130])))
    while sum(sizes) > N_REF_E - 40:
        sizes.pop()
    perm = rng.permutation(N_REF_E)
    ref_edges, at, members = [], 0, []
    for s in sizes:
        v = perm[at:at + s]
        members.append(v)
        at += s
        for k in range(1, s):
            ref_edges.append((v[k], v[rng.integers(0, k)]))
        for _ in range(s // 3):
            a, b = rng.choice(v, 2, replace=False)
            ref_edges.append((a, b))
    members += [perm[k:k + 1] for k in range(at, N_REF_E)]
    ref_edges = np.array(ref_edges, dtype=np.int64)
    pick = lambda c: int(rng.choice(members[c]))           # noqa: E731
    new, n_comp = [], len(members)
    for q in range(N_QRY_E):
        v, kind = N_REF_E + q, q % 8
        if kind == 1:
            new += [(pick(q % n_comp), v)] * (1 + q % 3)                              # singly linked, maybe repeated
        elif kind == 2:
            new += [(v, pick(q % n_comp)), (pick((q * 7) % n_comp), v)]               # merges two
        elif kind == 3:
            new += [(pick(c % n_comp), v) for c in (q, q * 5 + 1, q * 11 + 2)]        # merges three
        elif kind == 4 and q + 8 < N_QRY_E:
            new += [(pick(q % n_comp), v), (v, v + 8)]                                # a query-query chain ...
        elif kind == 5 and q >= 100:
            new += [(v, v - 8)] if q - 8 >= 100 else []                               # clusters of queries only
        elif kind == 6 and q + 8 < N_QRY_E:
            new += [(v + 8, v)]
    new = np.array(new, dtype=np.int64)
    new = new[rng.permutation(new.shape[0])]
    return ref_edges, new


EXTEND = extend_input()


def scipy_labels(edges, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    return connected_components(coo_matrix((np.ones(edges.shape[0]), (edges[:, 0], edges[:, 1])), shape=(n, n)),
                                directed=False)[1].astype(np.int32)


@pytest.fixture(scope="module")
def extend_reference():
    ref_edges, new = EXTEND
    full = np.concatenate([ref_edges, new])
    want, count = ranking_restated(N_REF_E + N_QRY_E, full[:, 0], full[:, 1])
    return want, count, scipy_labels(ref_edges, N_REF_E)


def test_extend_matches_the_full_graph_route_and_scipy(extend_reference):
    ref_edges, new = EXTEND
    want, count, label = extend_reference
    n = N_REF_E + N_QRY_E
    full_numbers, full_count = engine.cluster_numbers_dev(dev(np.concatenate([ref_edges, new])), n)
    assert np.array_equal(full_numbers.cpu().numpy(), want) and full_count == count
    got, got_count = engine.cluster_extend_dev(dev(new), dev(label), N_QRY_E)
    assert got.dtype == torch.int32 and got_count == count
    assert got.cpu().numpy().tobytes() == full_numbers.cpu().numpy().tobytes()
    assert np.array_equal(extend_restated(new[:, 0], new[:, 1], label, N_QRY_E)[0], want)
    # the same partition under other label values: any numbers in [0, n_ref)
    other = np.random.default_rng(9).permutation(N_REF_E).astype(np.int32)[label]
    got2, count2 = engine.cluster_extend_dev(dev(new), dev(other), N_QRY_E)
    assert count2 == count and got2.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    # the same call on a reshuffled, re-oriented stream: the same bits
    again = new[np.random.default_rng(10).permutation(new.shape[0])][:, ::-1].copy()
    got3, _ = engine.cluster_extend_dev(dev(again), dev(label), N_QRY_E)
    assert got3.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    host, host_count = network.cluster_extend(new[:, 0], new[:, 1], label, N_QRY_E)
    assert np.array_equal(host, want) and host_count == count


def test_extend_reads_the_reference_network_through_its_labels_alone(extend_reference):
    """every kind of query is in the input, and the seeded forest needs no reference edge"""
    ref_edges, new = EXTEND
    want, _, label = extend_reference
    deg = np.bincount(new.ravel(), minlength=N_REF_E + N_QRY_E)[N_REF_E:]
    assert (deg == 0).sum() >= 30 and (new.min(axis=1) >= N_REF_E).sum() >= 60
    sizes_before = np.bincount(ranking_restated(N_REF_E, ref_edges[:, 0], ref_edges[:, 1])[0])
    assert np.bincount(want).max() > sizes_before.max()      # components were merged
    only_queries = [c for c in np.unique(want[N_REF_E:]) if not (want[:N_REF_E] == c).any()
                    and (want[N_REF_E:] == c).sum() > 1]
    assert only_queries


def test_extend_without_queries_and_without_edges(extend_reference):
    ref_edges, _ = EXTEND
    _, _, label = extend_reference
    none = np.zeros((0, 2), dtype=np.int64)
    want, count = ranking_restated(N_REF_E, ref_edges[:, 0], ref_edges[:, 1])
    got, got_count = engine.cluster_extend_dev(dev(none), dev(label), 0)                  # n_qry = 0, n_edges = 0
    assert np.array_equal(got.cpu().numpy(), want) and got_count == count
    more = np.array([(3, 4), (10, 900)], dtype=np.int64)                                  # n_qry = 0 with edges
    full = np.concatenate([ref_edges, more])
    got, _ = engine.cluster_extend_dev(dev(more), dev(label), 0)
    assert np.array_equal(got.cpu().numpy(), ranking_restated(N_REF_E, full[:, 0], full[:, 1])[0])
    got, got_count = engine.cluster_extend_dev(dev(none), dev(label), 7)                  # n_edges = 0
    want7, count7 = ranking_restated(N_REF_E + 7, ref_edges[:, 0], ref_edges[:, 1])
    assert np.array_equal(got.cpu().numpy(), want7) and got_count == count7 == count + 7
    got, got_count = engine.cluster_extend_dev(dev(np.array([(0, 1)], dtype=np.int64)),   # n_ref = 0
                                               dev(np.zeros(0, dtype=np.int32)), 3)
    assert got.cpu().numpy().tolist() == [1, 1, 2] and got_count == 2


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_first_offender():
    label = np.zeros(10, dtype=np.int32)
    good = np.array([(0, 10), (1, 11), (2, 12)], dtype=np.int64)
    calls = {"ppk_query_links": lambda e, lab, nq: engine.query_links_dev(dev(e), dev(lab), nq, 4),
             "ppk_cluster_extend": lambda e, lab, nq: engine.cluster_extend_dev(dev(e), dev(lab), nq)}
    for who, call in calls.items():
        bad = label.copy()
        bad[[4, 7]] = [10, -1]
        with pytest.raises(RuntimeError, match=who + r": reference 4: label 10 outside \[0, 10\)"):
            call(good, bad, 3)
        e = good.copy()
        e[1] = (1, 13)
        with pytest.raises(RuntimeError, match=who + r": edge 1 \(i=1, j=13.*\): vertex id out of range \[0, 13\)"):
            call(e, label, 3)
        e[1] = (-1, 11)
        with pytest.raises(RuntimeError, match=who + r": edge 1 \(i=-1, j=11.*\): vertex id out of range"):
            call(e, label, 3)
        e[1], e[2] = (1, 11), (12, 12)
        with pytest.raises(RuntimeError, match=who + r": edge 2 \(i=12, j=12.*\): self-loop"):
            call(e, label, 3)
        call(good, label, 3)                                 # and the next call is clean
    for ml in (0, 65):
        with pytest.raises(RuntimeError, match="ppk_query_links: max_links must be 1 .. 64"):
            engine.query_links_dev(dev(good), dev(label), 3, ml)
    with pytest.raises(RuntimeError, match=r"ppk_query_links: n_ref \+ n_qry must be < 2\^31"):
        engine.query_links_dev(dev(good), dev(label), 2 ** 31 - 10, 4)
    with pytest.raises(RuntimeError, match=r"ppk_cluster_extend: n_ref \+ n_qry must be < 2\^31"):
        engine.cluster_extend_dev(dev(good), dev(label), 2 ** 31 - 10)
    with pytest.raises(TypeError):
        engine.query_links_dev(dev(good), dev(label.astype(np.int64)), 3, 4)


# ---- the reference-derived fixture, end to end ----------------------------------------------------------------------
def golden_model():
    return models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=DOC["x_max"], optimal_y=DOC["y_max"])


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("where", ["host_arrays", "device_tensors"])
def test_every_golden_case_end_to_end(name, where, tmp_path, capsys):
    case = CASES[name]
    got = run_golden_case(case, arrays(), tmp_path, capsys, golden_model(), dev if where == "device_tensors" else None)
    check_golden_case(case, got, tmp_path)


# ---- which route ran ---------------------------------------------------------------------------------------------------
def stages_of(call):
    """the ppk_prof_stages names one call reports"""
    import ctypes as C
    from poppunk_amd import _lib
    lib = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    lib.ppk_prof_stages_enable(1)
    try:
        lib.ppk_prof_stages_read(buf, len(buf), 1)
        call()
        torch.cuda.synchronize()
        lib.ppk_prof_stages_read(buf, len(buf), 1)
    finally:
        lib.ppk_prof_stages_enable(0)
    return [line.split("\t")[0] for line in buf.value.decode().splitlines()]


def test_the_ordered_stream_is_not_sorted_and_the_shuffled_one_is():
    """the two routes give the same bits, so only the stages tell which one ran"""
    label, ordered, mixed = LINKS
    lab_t = dev(label)
    # row order, with queries of 130 and 150 components: segments, the wave kernel, then the overflow list's sort
    assert stages_of(lambda: engine.query_links_dev(dev(ordered), lab_t, N_QRY_L, 4)) == \
        ["validate", "segments", "links", "overflow", "sort"]
    # row order, nobody over the set's capacity (queries 2 and 3 left out): nothing is sorted
    small = ordered[(ordered[:, 1] != N_REF_L + 2) & (ordered[:, 1] != N_REF_L + 3)]
    want = links_restated(small[:, 0], small[:, 1], label, N_QRY_L, 4)
    assert want[1].max() == 128                              # query 4 fills the set exactly and stays in it
    assert stages_of(lambda: engine.query_links_dev(dev(small), lab_t, N_QRY_L, 4)) == ["validate", "segments", "links"]
    got = got_links(small, label, N_QRY_L, 4)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # ... also with the skipped edges behind them, and in the other orientation
    tail = np.array([(0, 1), (N_REF_L, N_REF_L + 1)], dtype=np.int64)
    assert stages_of(lambda: engine.query_links_dev(dev(np.concatenate([small, tail])[:, ::-1]), lab_t, N_QRY_L,
                                                    4)) == ["validate", "segments", "links"]
    # any other order: a key per edge and the sort, for every query
    assert stages_of(lambda: engine.query_links_dev(dev(mixed), lab_t, N_QRY_L, 4)) == ["validate", "keys", "sort"]
    # the producers' order IS row order: the fused path's and generate_tuples' query-reference lists
    a = np.zeros(N_QRY_L * N_REF_L, dtype=np.int32)
    a[::37] = -1
    edges = engine.generate_tuples_dev(dev(a), -1, False, N_REF_L)
    assert stages_of(lambda: engine.query_links_dev(edges, lab_t, N_QRY_L, 4)) == ["validate", "segments", "links"]
    ref_edges, new = EXTEND
    assert stages_of(lambda: engine.cluster_extend_dev(dev(new), dev(scipy_labels(ref_edges, N_REF_E)), N_QRY_E)) == \
        ["validate", "csr", "clusters"]


# ---- weights on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance_type", ["core", "accessory", "euclidean"])
def test_device_weights_equal_the_numpy_route(distance_type, capsys):
    """addQueryToNetwork with weights on CUDA tensors (engine.edge_weights_dev for the query-reference rectangle and,
    with int_offset = n_ref, for the query-query triangle) against the same call on numpy arrays"""
    case, z = CASES["joint_unlinked"], arrays()
    qr, qq = z["joint_unlinked_qr"], z["joint_unlinked_qq"]
    # (distance_type 'core' / 'accessory' assign the query-query distances under slope 0 / 1: make_golden_assign.py's
    # boundaries for those)
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=DOC["x_max"], optimal_y=DOC["y_max"],
                                  core_boundary=DOC["x_max"] / 2, accessory_boundary=DOC["x_max"])
    ref_edges = np.array(DOC["ref_edges"], dtype=np.int64)
    old_w = np.linspace(0.001, 0.002, ref_edges.shape[0]).astype(np.float32)
    out = {}
    for where, put in (("host", lambda x: x), ("device", dev)):
        G, qqDistMat = network.addQueryToNetwork({'queryDatabase': lambda **kw: put(qq)}, DOC["rNames"], case["qNames"],
                                                 (put(ref_edges), N_REF, put(old_w)), model.assign(qr) if where == "host"
                                                 else model.assign_dev(dev(qr)), model, "db", kmers=[13],
                                                 distance_type=distance_type, weights=put(qr))
        out[where] = [np.asarray(x.cpu() if where == "device" else x) for x in (G[0], G[2])]
        assert G[1] == N_REF + 12 and (where == "host" or (G[0].is_cuda and G[2].is_cuda and G[2].dtype == torch.float32))
    if distance_type == "euclidean":                         # (the slope the fixture's network was built under)
        assert out["host"][0].tolist() == case["expected"]["network_edges"]
    assert np.array_equal(out["host"][0], out["device"][0])
    assert out["host"][1].astype(np.float32).tobytes() == out["device"][1].tobytes()
    # the weights are the rows the edges came from: query-query edges first, then query-reference, then the old ones
    e, w = out["device"]
    col = {"core": lambda d: d[:, 0], "accessory": lambda d: d[:, 1], "euclidean": lambda d: np.linalg.norm(d, axis=1)}
    is_qq = e.min(axis=1) >= N_REF
    is_qr = (e.min(axis=1) < N_REF) & (e.max(axis=1) >= N_REF)
    assert is_qq.sum() > 0 and is_qr.sum() > 0
    a, b = e[is_qq].min(axis=1) - N_REF, e[is_qq].max(axis=1) - N_REF
    assert np.array_equal(w[is_qq], col[distance_type](qq[a * 12 - a * (a + 1) // 2 + (b - a - 1)]))
    assert np.array_equal(w[is_qr], col[distance_type](qr[(e[is_qr].max(axis=1) - N_REF) * N_REF + e[is_qr].min(axis=1)]))
    assert np.array_equal(w[~is_qq & ~is_qr], old_w)


def test_graph_weights_in_assign_query_clusters(tmp_path, capsys):
    case, z = CASES["joint_unlinked"], arrays()
    qr, qq = z["joint_unlinked_qr"], z["joint_unlinked_qq"]
    ref_edges = np.array(DOC["ref_edges"], dtype=np.int64)
    old_w = np.full(ref_edges.shape[0], 0.5, dtype=np.float32)
    old = str(tmp_path / "old.csv")
    open(old, "w").write(DOC["old_csv"])
    got = {}
    for where, put in (("host", lambda x: x), ("device", dev)):
        output = str(tmp_path / where)
        os.makedirs(output)
        refnet = assign.ReferenceNetwork((put(ref_edges), N_REF, put(old_w)), DOC["rNames"], old)
        res = assign.assign_query_clusters({'queryDatabase': lambda **kw: put(qq)}, refnet, case["qNames"], put(qr),
                                           golden_model(), output, kmers=[13], graph_weights=True, return_network=True)
        assert res["isolateClustering"]["combined"] == case["expected"]["clustering"]
        e, n, w = res["genomeNetwork"]
        got[where] = (np.asarray(e.cpu() if where == "device" else e), np.asarray(w.cpu() if where == "device" else w))
        assert n == N_REF + 12 and got[where][0].tolist() == case["expected"]["network_edges"]
    assert got["host"][1].astype(np.float32).tobytes() == got["device"][1].tobytes()
    # a loaded network without weights: the reference's message and exit
    refnet = assign.ReferenceNetwork((dev(ref_edges), N_REF), DOC["rNames"], old)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        assign.assign_query_clusters({'queryDatabase': None}, refnet, case["qNames"], dev(qr), golden_model(),
                                     str(tmp_path / "host"),
                                     kmers=[13], graph_weights=True)
    assert "Loaded network does not have edge weights" in capsys.readouterr().err


# ---- straight from sketches ------------------------------------------------------------------------------------------
def test_assign_from_sketches_matches_the_matrix_route(tmp_path, capsys):
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, member = synth.make_sketches(370, kmers, cluster_size=30, seed=21)       # 12 clusters, member = k % 12
    # references: 300 samples of clusters 0 .. 9; queries: the 10 left of those clusters and 60 of clusters 10 and 11,
    # which no reference belongs to
    in_ref = np.flatnonzero(member < 10)
    ref_sk = np.ascontiguousarray(sk[in_ref[:300]])
    qry_sk = np.ascontiguousarray(sk[np.concatenate([in_ref[300:], np.flatnonzero(member >= 10)])])
    ref_db, qry_db = engine.SketchDB(ref_sk, 16, 14, device=0), engine.SketchDB(qry_sk, 16, 14, device=0)
    rNames, qNames = ["r%03d" % k for k in range(300)], ["q%02d" % k for k in range(70)]
    rr, _ = engine.dist(ref_db, None, kmers, tbl)
    x_max, y_max = synth.boundary_for_quantile(rr.cpu().numpy(), 0.03)
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max)
    ref_edges = engine.generate_tuples_dev(model.assign_dev(rr).to(torch.int32).contiguous(), model.within_label)
    fit_dir = tmp_path / "fit"
    os.makedirs(str(fit_dir))
    network.printClusters((ref_edges, 300), rNames, outPrefix=str(fit_dir / "fit"), write_unwords=False)
    old = str(fit_dir / "fit_clusters.csv")
    refnet = assign.ReferenceNetwork((ref_edges, 300), rNames, old)

    qr, _ = engine.dist(ref_db, qry_db, kmers, tbl)
    qq, _ = engine.dist(qry_db, None, kmers, tbl)
    out_a, out_b = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(out_a)
    os.makedirs(out_b)
    capsys.readouterr()
    want = assign.assign_query_clusters({'queryDatabase': lambda **kw: qq.cpu().numpy()}, refnet, qNames,
                                        qr.cpu().numpy(), model, out_a, kmers=kmers.tolist(), write_references=True)
    err_a = capsys.readouterr().err
    got, merged = assign.assign_from_sketches(ref_db, qry_db, model, refnet, qNames, kmers, tbl, out_b,
                                              write_references=True)
    err_b = capsys.readouterr().err
    ref_db.close()
    qry_db.close()
    assert "Found novel query clusters" in err_a             # the shape was chosen so that a query is novel
    assert got == want["isolateClustering"]["combined"] and sorted(merged) == sorted(want["merged_queries"])
    assert err_a == err_b
    assert open(os.path.join(out_a, "a_clusters.csv")).read() == open(os.path.join(out_b, "b_clusters.csv")).read()
