"""GPU tests of the query batch added to the lineages of every strain (ppk_strain_extend*, the tie-run lookup of
ppk_strain_ranks_dev, engine.strain_extend_dev, lineages.extend_strain_lineages).  Everything is
compared bit for bit with the numpy restatement (tests/strain_extend_model.py: oracle.extend and oracle.lower_rank strain
by strain) and with a loop over the calls that take one strain (ppk_extend, ppk_lower_rank); there are no tolerances.

Strain s has n_s members and q_s queries; a row of the extended strain has n_s + q_s - 1 candidates, which is what the
routes go by: 64 is the longest wave-route row, 65 the shortest LDS one, and option lineage_lds_keys 128 / 64 sends 129
and 300 / everything past 64 through the long route."""
import ctypes as C
import functools

import numpy as np
import pytest

import lineage_model
import strain_extend_model as model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, lineages, models, poppunk_refine  # noqa: E402

DEV = "cuda:0"
FLOOR = 1e-10
# (n_s, q_s): q_s 0, 1, 2 and n_s + 3 on a strain of 2; 64 / 65 / 128 / 129 / 300 candidates a row; a plain strain of 10
SHAPES = [(2, 0), (2, 1), (2, 2), (2, 5), (60, 5), (60, 6), (120, 9), (120, 10), (290, 11), (10, 0)]
N_REF, N_QRY = 700, 60


def as_dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_lists(got, want, what=""):
    for g, w, name in zip(got[:2], want[:2], "ij"):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, name)
    assert got[2].dtype == np.float32 and np.array_equal(bits(got[2]), bits(want[2])), (what, "dist")


def long_index(a, b, n):
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * (2 * n - lo - 1) // 2 + (hi - lo - 1)


def make_case(shapes, n_ref, n_qry, seed, depth, col=0, copies=True):
    """Members and queries interleaved in id space and shuffled; some samples and queries (those of a strain without a
    model) in no list.  Column 0 is quantised to 1/64 (many ties), column 1 nearly all distinct.  With `copies`, every
    third query is a copy of a member of its strain (distance 0 to it, the member's distances otherwise), the last two
    queries of a strain with at least four are copies of each other, and a -0.0 stands in both matrices."""
    rng = np.random.default_rng(seed)
    perm, qperm = rng.permutation(n_ref).astype(np.int64), rng.permutation(n_qry).astype(np.int64)
    seg_off = np.concatenate([[0], np.cumsum([n for n, _ in shapes])]).astype(np.int64)
    qry_off = np.concatenate([[0], np.cumsum([q for _, q in shapes])]).astype(np.int64)
    assert seg_off[-1] < n_ref and qry_off[-1] < n_qry
    members, queries = perm[:seg_off[-1]].copy(), qperm[:qry_off[-1]].copy()

    def values(rows):
        d = rng.random((rows, 2)).astype(np.float32)
        d[:, 0] = np.floor(d[:, 0] * 64) / 64
        d[rng.integers(0, rows, max(rows // 50, 1)), 1] = 0.0
        return d
    rr, qr, qq = values(n_ref * (n_ref - 1) // 2), values(n_qry * n_ref), values(n_qry * (n_qry - 1) // 2)
    if copies:
        for s, (n_s, q_s) in enumerate(shapes):
            mem, qry = members[seg_off[s]:seg_off[s + 1]], queries[qry_off[s]:qry_off[s + 1]]
            for k in range(0, q_s, 3):
                twin = mem[(k * 7) % n_s]
                others = mem[mem != twin]
                qr[qry[k] * n_ref + others] = rr[long_index(twin, others, n_ref)]
                qr[qry[k] * n_ref + twin] = 0.0
            if q_s >= 4:
                a, b = qry[-1], qry[-2]
                qr[a * n_ref + mem] = qr[b * n_ref + mem]
                rest = qry[:-2]
                qq[long_index(a, rest, n_qry)] = qq[long_index(b, rest, n_qry)]
                qq[long_index(a, b, n_qry)] = 0.0
        one = next(s for s, (_, q_s) in enumerate(shapes) if q_s >= 1)
        two = next(s for s, (_, q_s) in enumerate(shapes) if q_s >= 2)
        qr[queries[qry_off[one]] * n_ref + members[seg_off[one]]] = -0.0
        qq[long_index(queries[qry_off[two]], queries[qry_off[two] + 1], n_qry)] = -0.0
    # the stored lists as a fitted model holds them: floored (models.LineageRanks._coo)
    stored = lineage_model.strain_knn(rr, n_ref, members, seg_off, depth, col)
    stored = (stored[0], stored[1], np.maximum(stored[2], np.float32(FLOOR)))
    return dict(members=members, seg_off=seg_off, queries=queries, qry_off=qry_off, stored=stored, qr=qr, qq=qq,
                n_ref=n_ref, n_qry=n_qry, depth=depth, col=col, rr=rr)


def run_extend(case, **changes):
    c = dict(case, **changes)
    got = engine.strain_extend_dev(as_dev(c["members"], np.int64), c["seg_off"], as_dev(c["queries"], np.int64),
                                   c["qry_off"], as_dev(c["stored"][1], np.int64), as_dev(c["stored"][2], np.float32),
                                   as_dev(c["qr"], np.float32), None if c["qq"] is None else as_dev(c["qq"], np.float32),
                                   c["n_ref"], c["n_qry"], c["depth"], c["col"], FLOOR)
    return tuple(t.cpu().numpy() for t in got)


def want_extend(case):
    c = case
    return model.strain_extend(c["members"], c["seg_off"], c["queries"], c["qry_off"], c["stored"], c["qr"], c["qq"],
                               c["n_ref"], c["n_qry"], c["depth"], c["col"], FLOOR)


@functools.lru_cache(maxsize=None)
def big_case(depth, col):
    case = make_case(SHAPES, N_REF, N_QRY, 31, depth, col)
    return case, want_extend(case)


@pytest.mark.parametrize("col", [0, 1])
@pytest.mark.parametrize("depth", [8, 10000])
def test_shapes_and_depths(depth, col):
    """depth 8 truncates the stored rows of every strain past 9 members; 10 000 keeps every row whole."""
    case, want = big_case(depth, col)
    got = run_extend(case)
    assert len(got[0]) == engine.strain_nnz(case["seg_off"] + case["qry_off"], depth)
    assert_lists(got, want, "depth %d, column %d" % (depth, col))
    assert not np.signbit(got[2]).any() and (got[2] >= np.float32(FLOOR)).all()
    # a strain without queries comes back as its stored lists
    nn_off, out_off = model.stored_offsets(case["seg_off"], depth), model.stored_offsets(
        case["seg_off"] + case["qry_off"], depth)
    for s in (0, len(SHAPES) - 1):
        for g, w in zip(got, case["stored"]):
            assert np.array_equal(g[out_off[s]:out_off[s + 1]], w[nn_off[s]:nn_off[s + 1]])


@pytest.mark.parametrize("options", [{"lineage_lds_keys": 128}, {"lineage_lds_keys": 128, "lineage_scratch_mb": 1},
                                     {"lineage_lds_keys": 64, "lineage_scratch_mb": 0}])
@pytest.mark.parametrize("depth", [8, 10000])
def test_routes(options, depth, ppk_option):
    """lineage_lds_keys 128 keeps 65 and 128 candidates in LDS and sends 129 and 300 through the long route (64: all
    four); one MiB of scratch cuts the 301 rows of 300 keys into two bands (174 rows fit), none gives bands of a row."""
    case, want = big_case(depth, 0)
    for name, value in options.items():
        ppk_option(name, value)
    assert_lists(run_extend(case), want, str(options))


def test_depth_equal_to_the_extended_row():
    """One strain of 12 members and 4 queries at depth 15 = n'_s - 1 (stored rows whole: min(15, 11) entries), and at
    14 and 11."""
    for depth in (15, 14, 11):
        case = make_case([(12, 4)], 40, 9, 7, depth)
        got = run_extend(case)
        assert len(got[0]) == 16 * min(depth, 15)
        assert_lists(got, want_extend(case), "depth %d" % depth)


def test_equals_the_single_strain_calls():
    """Strain by strain: ppk_extend on the strain's stored triplets, floored square and floored rectangle, knn = depth."""
    case, _ = big_case(8, 0)
    got = run_extend(case)
    out_off = model.stored_offsets(case["seg_off"] + case["qry_off"], 8)
    for s in range(len(SHAPES)):
        trip, square, rect = model.strain_inputs(s, case["members"], case["seg_off"], case["queries"], case["qry_off"],
                                                 case["stored"], case["qr"], case["qq"], N_REF, N_QRY, 8, 0, FLOOR)
        want = poppunk_refine.extend_arrays(trip, square, rect, 8)
        want = (np.asarray(want[0], dtype=np.int64), np.asarray(want[1], dtype=np.int64),
                np.asarray(want[2], dtype=np.float32))
        assert_lists(tuple(a[out_off[s]:out_off[s + 1]] for a in got), want, "strain %d" % s)


def tie_case():
    """A strain of 50 members and 40 queries all at one distance (the floor): every row is one run of 89 equal
    distances, the 40 queries (columns 50 ..) before the stored columns; beside it a strain of identical genomes among
    distinct ones."""
    case = make_case([(50, 40), (30, 8)], 100, 60, 3, 10000)
    case["qr"][:] = 0.0
    case["qq"][:] = 0.0
    case["qq"][::7] = -0.0
    rr = case["rr"]
    mem = case["members"][:50]
    a, b = np.triu_indices(50, 1)
    rr[long_index(mem[a], mem[b], 100)] = FLOOR
    stored = lineage_model.strain_knn(rr, 100, case["members"], case["seg_off"], 10000, 0)
    case["stored"] = (stored[0], stored[1], np.maximum(stored[2], np.float32(FLOOR)))
    # the second strain keeps random distances to its queries but for three copies of a member
    mem2, qry2 = case["members"][50:80], case["queries"][40:48]
    case["qr"][(qry2[:, None] * 100 + mem2[None, :]).ravel()] = np.random.default_rng(4).random((240, 2)).astype(np.float32)
    for k in range(3):
        others = mem2[mem2 != mem2[5]]
        case["qr"][qry2[k] * 100 + others] = rr[long_index(mem2[5], others, 100)]
        case["qr"][qry2[k] * 100 + mem2[5]] = 0.0
    return case


@functools.lru_cache(maxsize=None)
def tie_lists():
    case = tie_case()
    want = want_extend(case)
    got = run_extend(case)
    assert_lists(got, want, "tie case")
    j = got[1][:90 * 89].reshape(90, 89)
    for r in (0, 49):                    # a member's row: every query, then its stored row (columns ascending)
        assert j[r].tolist() == list(range(50, 90)) + [c for c in range(50) if c != r]
    for r in (50, 89):                   # a query's row: the other queries, then the members
        assert j[r].tolist() == [c for c in range(50, 90) if c != r] + list(range(50))
    return case, got


@pytest.mark.parametrize("ranks", [[1, 2, 5], [3, 45, 60]])      # 45 and 60 cut inside the run, on either side
@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("unique", [False, True])
def test_ranks_of_the_extended_lists(ranks, reciprocal, unique):
    """The mirror lookup of the level stream on lists in extend's order: inside a run of equal distances the query
    columns come before the stored ones, so the run is scanned, not bisected by column."""
    case, lists = tie_lists()
    ext_off = model.extended_segments(case["seg_off"], case["qry_off"])
    m = int(ext_off[-1])
    want_prefix, want_stream, want_numbers, _ = model.strain_extend_ranks(lists, case["seg_off"], case["qry_off"], 10000,
                                                                          ranks, reciprocal, unique, FLOOR)
    prefix, pi, pj, lv, sd = engine.strain_ranks_dev(as_dev(lists[1], np.int64), as_dev(lists[2], np.float32), ext_off,
                                                     10000, ranks, reciprocal, unique, FLOOR)
    assert np.array_equal(prefix.cpu().numpy(), want_prefix)
    a, b, level = pi.cpu().numpy(), pj.cpu().numpy(), lv.cpu().numpy()
    got = np.stack([np.minimum(a, b), np.maximum(a, b), level], axis=1)
    got = got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))]
    assert len(np.unique(got[:, :2], axis=0)) == len(got), "an unordered pair is in the stream twice"
    assert np.array_equal(got, want_stream)
    clusters, _ = engine.cluster_sweep_dev(pi, pj, lv, m, len(ranks))
    assert np.array_equal(engine.strain_cluster_numbers(clusters, ext_off).cpu().numpy(), want_numbers)


def test_ranks_of_the_big_case_equal_lower_rank_per_strain():
    """ppk_lower_rank strain by strain on the extended lists (ranks 1, 2, 5 at depth 8; reciprocal and unique counting)."""
    case, lists = big_case(8, 0)
    ext_off = model.extended_segments(case["seg_off"], case["qry_off"])
    out_off = model.stored_offsets(ext_off, 8)
    for reciprocal, unique in ((False, False), (True, True)):
        prefix, pi, pj, lv, sd = engine.strain_ranks_dev(as_dev(lists[1], np.int64), as_dev(lists[2], np.float32),
                                                         ext_off, 8, [1, 2, 5], reciprocal, unique, FLOOR)
        want_prefix, want_stream, _, _ = model.strain_extend_ranks(lists, case["seg_off"], case["qry_off"], 8, [1, 2, 5],
                                                                   reciprocal, unique, FLOOR)
        assert np.array_equal(prefix.cpu().numpy(), want_prefix)
        a, b, level = pi.cpu().numpy(), pj.cpu().numpy(), lv.cpu().numpy()
        got = np.stack([np.minimum(a, b), np.maximum(a, b), level], axis=1)
        assert np.array_equal(got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))], want_stream)
        for s in (3, 5, 8):
            trip = tuple(x[out_off[s]:out_off[s + 1]] for x in lists)
            n_x = int(ext_off[s + 1] - ext_off[s])
            for q, rank in enumerate([1, 2, 5]):
                if rank >= n_x:
                    continue
                li, lj, ld = poppunk_refine.lowerRank_arrays(trip, n_x, rank, reciprocal, unique, FLOOR)
                if reciprocal:
                    keep = (lv.cpu().numpy() <= q) & (a >= ext_off[s]) & (a < ext_off[s + 1])
                    assert np.array_equal(a[keep] - ext_off[s], li) and np.array_equal(b[keep] - ext_off[s], lj)
                    assert np.array_equal(bits(sd.cpu().numpy()[keep]), bits(ld))
                else:
                    assert np.array_equal(np.bincount(np.asarray(li), minlength=n_x),
                                          want_prefix[q, ext_off[s]:ext_off[s + 1]])


def local_long(dist, n, mem):
    a, b = np.triu_indices(len(mem), 1)
    return np.ascontiguousarray(dist[long_index(mem[a], mem[b], n)])


def same_coo(got, want, what):
    assert got.shape == want.shape, what
    for name in ("row", "col"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)
    assert got.data.dtype == want.data.dtype and np.array_equal(bits(got.data), bits(want.data)), (what, "data")


@pytest.mark.parametrize("flags", [dict(), dict(reciprocal_only=True, count_unique_distances=True, use_accessory=True,
                                                max_search_depth=8, ranks=[1, 2, 5])])
def test_fit_then_extend_equals_the_single_strain_model(flags):
    """fit_strain_lineages -> extend_strain_lineages against LineageRanks.fit -> .extend one strain at a time, array for
    array, numbers included.  strain0 is below min_count (no model: its query is left out), strain3 gets no query."""
    shapes = [(9, 1), (10, 1), (30, 2), (12, 0), (66, 13)]
    case = make_case(shapes, 200, 25, 41, 10000)
    rr, seg_off, qry_off, members, queries = (case[k] for k in ("rr", "seg_off", "qry_off", "members", "queries"))
    rnames, qnames = ["s%03d" % k for k in range(200)], ["q%02d" % k for k in range(25)]
    strain_of = {"strain%d" % s: [rnames[g] for g in members[seg_off[s]:seg_off[s + 1]]] for s in range(len(shapes))}
    strain_of_query = {qnames[q]: "strain%d" % s for s in range(len(shapes)) for q in queries[qry_off[s]:qry_off[s + 1]]}
    flags = dict(flags)
    ranks = flags.pop("ranks", [1, 2, 3])
    fitted = lineages.fit_strain_lineages(as_dev(rr, np.float32), rnames, strain_of, ranks, min_count=10, **flags)
    loaded = {strain: entry[0] for strain, entry in fitted.items()}
    names_of = {strain: strain_of[strain] for strain in loaded}
    got = lineages.extend_strain_lineages(loaded, names_of, qnames, strain_of_query, as_dev(case["qr"], np.float32),
                                          as_dev(case["qq"], np.float32), rnames)
    assert list(got) == ["strain1", "strain2", "strain4"]
    col = 1 if flags.get("use_accessory") else 0
    for s in (1, 2, 4):
        mem, qry = members[seg_off[s]:seg_off[s + 1]], np.sort(queries[qry_off[s]:qry_off[s + 1]])     # qNames' order
        single = models.LineageRanks(ranks, flags.get("max_search_depth", 10000), flags.get("reciprocal_only", False),
                                     flags.get("count_unique_distances", False), dist_col=col)
        single.fit(local_long(rr, 200, mem))
        if len(qry) > 1:
            single.extend(local_long(case["qq"], 25, qry), case["qr"][(qry[:, None] * 200 + mem[None, :]).ravel()])
        else:
            # LineageRanks.extend reads the number of queries off the long form, which cannot state one: its steps
            rect = np.maximum(case["qr"][qry[None, :] * 200 + mem[:, None], col], np.float32(FLOOR))
            higher = poppunk_refine.extend_arrays((single.nn_dists.row, single.nn_dists.col, single.nn_dists.data),
                                                  np.full((1, 1), FLOOR, dtype=np.float32), rect,
                                                  single.max_search_depth)
            single.nn_dists = single._coo(higher[2], higher[0], higher[1], len(mem) + 1)
            single._ranks_from(higher, len(mem) + 1)
        new, clusters, overall = got["strain%d" % s]
        assert new is not loaded["strain%d" % s]
        same_coo(new.nn_dists, single.nn_dists, "nn_dists of strain %d" % s)
        isolates = strain_of["strain%d" % s] + [qnames[q] for q in qry]
        for rank in ranks:
            same_coo(new.lower_rank_dists[rank], single.lower_rank_dists[rank], "rank %d of strain %d" % (rank, s))
            edges = np.stack([single.lower_rank_dists[rank].row, single.lower_rank_dists[rank].col], axis=1)
            want = lineage_model.print_clusters_numbers(lineage_model.components(len(isolates), edges))
            assert [clusters[rank][name] for name in isolates] == want.tolist()
        assert list(overall) == ["Rank_%d" % r for r in ranks] + ["overall"]
        assert list(overall["overall"]) == list(clusters[ranks[0]])


def test_a_model_outside_the_layout_goes_alone(monkeypatch):
    """A model whose rows are not min(depth, n_s - 1) long goes through the calls that take one strain; on a model that
    is in the layout both routes give the same arrays and numbers."""
    shapes = [(20, 3), (30, 1)]
    case = make_case(shapes, 80, 10, 43, 10000)
    rnames, qnames = ["s%03d" % k for k in range(80)], ["q%02d" % k for k in range(10)]
    seg_off, qry_off, members, queries = (case[k] for k in ("seg_off", "qry_off", "members", "queries"))
    strain_of = {"strain%d" % s: [rnames[g] for g in members[seg_off[s]:seg_off[s + 1]]] for s in range(2)}
    strain_of_query = {qnames[q]: "strain%d" % s for s in range(2) for q in queries[qry_off[s]:qry_off[s + 1]]}
    fitted = lineages.fit_strain_lineages(as_dev(case["rr"], np.float32), rnames, strain_of, [1, 2], min_count=10)
    loaded = {strain: entry[0] for strain, entry in fitted.items()}
    args = (loaded, strain_of, qnames, strain_of_query, case["qr"], case["qq"], rnames)
    batch = lineages.extend_strain_lineages(*args)
    monkeypatch.setattr(lineages, "_stored_rows", lambda model, n_s: None)
    alone = lineages.extend_strain_lineages(*args)
    for strain in ("strain0", "strain1"):
        same_coo(alone[strain][0].nn_dists, batch[strain][0].nn_dists, strain)
        for rank in (1, 2):
            same_coo(alone[strain][0].lower_rank_dists[rank], batch[strain][0].lower_rank_dists[rank], (strain, rank))
        assert alone[strain][1] == batch[strain][1] and alone[strain][2] == batch[strain][2]
        assert [list(d) for d in alone[strain][1].values()] == [list(d) for d in batch[strain][1].values()]


@pytest.mark.parametrize("run", ["default", "flags"])
def test_golden_case_end_to_end(run, tmp_path, capsys, monkeypatch):
    """python -m poppunk_amd.lineages --create-db, then --query-db, on the golden case: the reference's files, arrays and
    dicts (lineage_query_golden.py says what is taken from the record and how the hash-ordered rows are compared)."""
    import lineage_query_golden
    lineage_query_golden.run_and_check(tmp_path, run, capsys, monkeypatch)


def test_host_form():
    case = make_case([(2, 1), (30, 4), (66, 0), (70, 9)], 200, 20, 13, 8, col=1)
    want = want_extend(case)
    nnz = engine.strain_nnz(case["seg_off"] + case["qry_off"], 8)
    oi, oj, od = np.zeros(nnz, dtype=np.int64), np.zeros(nnz, dtype=np.int64), np.zeros(nnz, dtype=np.float32)
    llp, fp = C.POINTER(C.c_longlong), C.POINTER(C.c_float)
    arr = lambda a, p: np.ascontiguousarray(a).ctypes.data_as(p)
    rc = _lib.lib().ppk_strain_extend(arr(case["members"], llp), arr(case["seg_off"], llp), arr(case["queries"], llp),
                                      arr(case["qry_off"], llp), 4, arr(case["stored"][1], llp),
                                      arr(case["stored"][2], fp), arr(case["qr"], fp), arr(case["qq"], fp), 200, 20, 1,
                                      FLOOR, 8, 0, oi.ctypes.data_as(llp), oj.ctypes.data_as(llp), od.ctypes.data_as(fp))
    _lib.check(rc, "ppk_strain_extend")
    assert_lists((oi, oj, od), want)


def test_errors_name_the_first_offender():
    case = make_case([(5, 2), (6, 1), (7, 3)], 100, 12, 9, 3, copies=False)
    members, queries, stored = case["members"], case["queries"], case["stored"]

    def fails(message, **changes):
        with pytest.raises(RuntimeError, match=message):
            run_extend(case, **changes)
    bad = members.copy()
    bad[7], bad[12] = 100, -1                                # strain 1, member 2 comes first
    fails(r"ppk_strain_extend: strain 1, member 2: sample 100 outside \[0, 100\)", members=bad)
    twice = members.copy()
    twice[13] = members[3]
    fails("ppk_strain_extend: strain 2, member 2: sample %d is already member 3 of strain 0" % members[3], members=twice)
    bad = queries.copy()
    bad[2], bad[4] = 12, -3                                  # strain 1, query 0 comes first
    fails(r"ppk_strain_extend: strain 1, query 0: query 12 outside \[0, 12\)", queries=bad)
    twice = queries.copy()
    twice[4] = queries[1]
    fails("ppk_strain_extend: strain 2, query 1: query %d is already query 1 of strain 0" % queries[1], queries=twice)
    # the stored lists: strain 1 starts at entry 15, three entries a row
    at = 15 + 2 * 3 + 1
    for value, what in ((6, r"column 6 outside \[0, 6\)"), (-1, r"column -1 outside \[0, 6\)"),
                        (2, "column 2 is the row itself")):
        j = stored[1].copy()
        j[at] = value
        fails("ppk_strain_extend: strain 1, row 2, entry 1: " + what, stored=(stored[0], j, stored[2]))
    d = stored[2].copy()
    d[at] = np.nextafter(d[at - 1], np.float32(0.0))
    d[at + 9] = 0.0
    fails("ppk_strain_extend: strain 1, row 2, entry 1: the distance is below the entry before it",
          stored=(stored[0], stored[1], d))
    # the members come before the queries, the queries before the stored lists
    bad_m, bad_q = members.copy(), queries.copy()
    bad_m[17], bad_q[0] = 100, 12
    fails("strain 2, member 6: sample 100", members=bad_m, queries=bad_q, stored=(stored[0], j, stored[2]))
    fails("strain 0, query 0: query 12", queries=bad_q, stored=(stored[0], j, stored[2]))
    fails("ppk_strain_extend: strain 0 has 2 queries and d_qq is NULL", qq=None)
    assert_lists(run_extend(case), want_extend(case))


def test_query_rows_are_indexed_in_64_bits():
    """q * n_ref + r on a database of 100 000 references and 30 000 queries: the last row is 2 999 999 999."""
    assert engine.qr_row_index(29999, 99999, 100000) == 2999999999
    assert engine.qr_row_index(np.int32(29999), np.int32(99999), np.int32(100000)) == 2999999999
