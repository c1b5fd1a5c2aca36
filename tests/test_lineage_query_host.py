"""Host tests of the query batch added to the lineages of every strain, no GPU: the numpy restatement
(tests/strain_extend_model.py) against a hand-worked case and against LineageRanks.extend's steps on the host oracle,
strain by strain; lineages.extend_strain_lineages' name, order, model and error logic with the restatement standing in
for the device; save -> load -> extend; the ABI entries and the errors that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import lineage_model
import strain_extend_model as model
from oracle import oracle
from poppunk_amd import _lib, engine, lineages, models

FLOOR = np.float32(1e-10)


def model_fit(dist, n, members, seg_off, depth, col, ranks, reciprocal_only, count_unique_distances, epsilon,
              device_id=0):
    lists = lineage_model.strain_knn(np.asarray(dist), n, members, seg_off, depth, col)
    _, _, numbers, outputs = lineage_model.strain_ranks(lists, seg_off, depth, ranks, reciprocal_only,
                                                        count_unique_distances, epsilon)
    sizes = np.diff(seg_off)
    return lineages._split(lists, sizes * np.minimum(depth, sizes - 1)), outputs, numbers


def model_extend(members, seg_off, queries, qry_off, stored, qr, qq, n_ref, n_qry, depth, col, ranks, reciprocal_only,
                 count_unique_distances, epsilon, device_id=0):
    """lineages._device_extend's contract, computed by the restatement."""
    sizes = np.diff(seg_off)
    rows = np.repeat(np.concatenate([np.arange(n) for n in sizes]), np.repeat(np.minimum(depth, sizes - 1), sizes))
    lists = model.strain_extend(members, seg_off, queries, qry_off, (rows, stored[0], stored[1]), np.asarray(qr),
                                None if qq is None else np.asarray(qq), n_ref, n_qry, depth, col, 1e-10)
    _, _, numbers, outputs = model.strain_extend_ranks(lists, seg_off, qry_off, depth, ranks, reciprocal_only,
                                                       count_unique_distances, epsilon)
    ext = np.diff(model.extended_segments(seg_off, qry_off))
    return lineages._split(lists, ext * np.minimum(depth, ext - 1)), outputs, numbers


@pytest.fixture
def on_model(monkeypatch):
    monkeypatch.setattr(lineages, "_device_fit", model_fit)
    monkeypatch.setattr(lineages, "_device_extend", model_extend)


def test_model_on_a_hand_worked_strain():
    """Three members on a line at 0, 2, 6 (distances |a - b| / 8) with stored lists of depth 2, and two queries: one at
    2 (a copy of member 1: distance 0 -> the floor) and one at 5."""
    stored = (np.asarray([0, 0, 1, 1, 2, 2]), np.asarray([1, 2, 0, 2, 1, 0]),
              np.asarray([2, 6, 2, 4, 4, 6], dtype=np.float32) / 8)
    x_ref, x_qry = np.asarray([0.0, 2.0, 6.0]), np.asarray([2.0, 5.0])
    qr = np.stack([np.abs(x_qry[:, None] - x_ref[None, :]).ravel() / 8] * 2, axis=1).astype(np.float32)
    qq = np.asarray([[3 / 8, 3 / 8]], dtype=np.float32)
    members, seg_off = np.arange(3), np.asarray([0, 3])
    queries, qry_off = np.asarray([0, 1]), np.asarray([0, 2])
    i, j, d = model.strain_extend(members, seg_off, queries, qry_off, stored, qr, qq, 3, 2, 2)
    assert i.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    # member 0: query 0 ties with member 1 at 2/8 and goes first; member 1: its copy at the floor, then member 0;
    # member 2: query 1 at 1/8, then query 0 before member 1, both at 4/8; query 0 (row 3): member 1 at the floor, then
    # member 0; query 1 (row 4): member 2 at 1/8, then 3/8 twice: the query side (query 0) before member 1
    assert j.tolist() == [3, 1, 3, 0, 4, 3, 1, 0, 2, 3]
    assert d.tolist() == [np.float32(2 / 8), np.float32(2 / 8), FLOOR, np.float32(2 / 8), np.float32(1 / 8),
                          np.float32(4 / 8), FLOOR, np.float32(2 / 8), np.float32(1 / 8), np.float32(3 / 8)]
    # a strain without queries comes back as it is
    none = model.strain_extend(members, seg_off, np.zeros(0, dtype=np.int64), np.asarray([0, 0]), stored, qr, None, 3, 2, 2)
    assert all(np.array_equal(a, b) for a, b in zip(none, stored))


def make_case(seed=5, n_ref=60, n_qry=14):
    """Strains of 12, 20 and 15 members (shuffled, interleaved); queries placed 3 / 0 / 5, two in a strain without a
    model ("x"), one in none; the first query of strain "a" is a copy of one of its members and the last two of "c" are
    copies of each other."""
    rng = np.random.default_rng(seed)
    rr = rng.random((n_ref * (n_ref - 1) // 2, 2)).astype(np.float32)
    rr[:, 0] = np.floor(rr[:, 0] * 16) / 16
    qr = rng.random((n_qry * n_ref, 2)).astype(np.float32)
    qr[:, 0] = np.floor(qr[:, 0] * 16) / 16
    qq = rng.random((n_qry * (n_qry - 1) // 2, 2)).astype(np.float32)
    rnames, qnames = ["r%02d.fa" % k for k in range(n_ref)], ["q%02d.fa" % k for k in range(n_qry)]
    perm = rng.permutation(n_ref)
    strain_of = {"a": [rnames[k] for k in perm[:12]], "b": [rnames[k] for k in perm[12:32]],
                 "c": [rnames[k] for k in perm[32:47]]}
    placing = {"a": [7, 2, 11], "c": [0, 13, 4, 9, 5], "x": [1, 3]}
    strain_of_query = {qnames[q]: s for s, qs in placing.items() for q in qs}
    twin = perm[3]
    others = np.asarray([k for k in perm[:12] if k != twin])
    lo, hi = np.minimum(twin, others), np.maximum(twin, others)
    qr[2 * n_ref + others] = rr[lo * (2 * n_ref - lo - 1) // 2 + (hi - lo - 1)]
    qr[2 * n_ref + twin] = 0.0
    qr[13 * n_ref:14 * n_ref] = qr[9 * n_ref:10 * n_ref]
    qq[9 * (2 * n_qry - 9 - 1) // 2 + (13 - 9 - 1)] = 0.0
    return rr, qr, qq, rnames, qnames, strain_of, strain_of_query


def oracle_extend_alone(fit, mem, qry, qr, qq, n_ref, n_qry):
    """LineageRanks.extend's steps (PopPUNK/models.py:1337-1389) for one strain with the oracle in the C++'s place."""
    col = fit.dist_col
    rect = np.maximum(qr[qry[None, :] * n_ref + mem[:, None], col], FLOOR)
    lo, hi = np.minimum(qry[:, None], qry[None, :]), np.maximum(qry[:, None], qry[None, :])
    off = np.where(lo != hi, lo * (2 * n_qry - lo - 1) // 2 + (hi - lo - 1), 0)
    square = np.maximum(np.where(lo != hi, qq[off, col], np.float32(0)), FLOOR).astype(np.float32)
    higher = oracle.extend(fit.nn_dists.row, fit.nn_dists.col, fit.nn_dists.data, square, rect, fit.max_search_depth)
    n_x = len(mem) + len(qry)
    out = {"nn": fit._coo(higher[2], higher[0], higher[1], n_x)}
    for rank in fit.ranks:
        low = oracle.lower_rank(higher[0], higher[1], higher[2], n_x, rank, fit.reciprocal_only,
                                fit.count_unique_distances, fit.resolution)
        out[rank] = fit._coo(low[2], low[0], low[1], n_x)
    return out


def same_coo(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got.row, want.row) and np.array_equal(got.col, want.col), what
    assert got.data.dtype == np.float32 and np.array_equal(got.data.view(np.uint32), want.data.view(np.uint32)), what


@pytest.mark.parametrize("flags", [dict(), dict(reciprocal_only=True, count_unique_distances=True, use_accessory=True,
                                                max_search_depth=8, ranks=[1, 2, 5])])
def test_extend_strain_lineages_on_the_model(flags, on_model, tmp_path):
    rr, qr, qq, rnames, qnames, strain_of, strain_of_query = make_case()
    flags = dict(flags)
    ranks = flags.pop("ranks", [1, 2, 3])
    fitted = lineages.fit_strain_lineages(rr, rnames, strain_of, ranks, min_count=10, **flags)
    # save -> load: what --query-db will read
    loaded = {}
    for strain, (fit, _, _) in fitted.items():
        prefix = str(tmp_path / ("strain_%s_lineage_db" % strain))
        os.makedirs(prefix)
        fit.save(prefix)
        loaded[strain] = models.LineageRanks.load(prefix)
    got = lineages.extend_strain_lineages(loaded, strain_of, qnames, strain_of_query, qr, qq, rnames)
    assert list(got) == ["a", "c"]                      # "b" has no query, "x" no model
    index = {name: k for k, name in enumerate(rnames)}
    for strain, placed in (("a", [2, 7, 11]), ("c", [0, 4, 5, 9, 13])):       # qNames' order
        new, clusters, overall = got[strain]
        mem = np.asarray([index[name] for name in strain_of[strain]])
        want = oracle_extend_alone(loaded[strain], mem, np.asarray(placed), qr, qq, len(rnames), len(qnames))
        same_coo(new.nn_dists, want["nn"], strain)
        isolates = strain_of[strain] + [qnames[q] for q in placed]
        for rank in ranks:
            same_coo(new.lower_rank_dists[rank], want[rank], (strain, rank))
            numbers = lineage_model.print_clusters_numbers(lineage_model.components(
                len(isolates), zip(want[rank].row, want[rank].col)))
            assert clusters[rank] == dict(zip(isolates, numbers.tolist()))
            values = list(clusters[rank].values())
            assert values == sorted(values)             # printClusters' order: lineage 1 first
        assert overall == lineages.createOverallLineage(ranks, clusters)
        assert (new.ranks, new.max_search_depth, new.dist_col) == (
            loaded[strain].ranks, loaded[strain].max_search_depth, loaded[strain].dist_col)
        # the loaded model is not touched, and the new one saves and loads
        assert loaded[strain].nn_dists.shape == (len(mem), len(mem))
        prefix = str(tmp_path / ("again_" + strain))
        os.makedirs(prefix)
        new.save(prefix)
        same_coo(models.LineageRanks.load(prefix).nn_dists, new.nn_dists, "saved again")
    # the sequence form of strain_of_query, and rows stored in another order inside a run of equal distances
    as_list = [strain_of_query.get(name) for name in qnames]
    again = lineages.extend_strain_lineages(loaded, strain_of, qnames, as_list, qr, qq, rnames)
    same_coo(again["c"][0].nn_dists, got["c"][0].nn_dists, "sequence form")
    coo = loaded["a"].nn_dists
    flip = np.arange(len(coo.row))[::-1]                # rows descending, every row's distances descending
    from scipy.sparse import coo_matrix
    loaded["a"].nn_dists = coo_matrix((coo.data[flip], (coo.row[flip], coo.col[flip])), shape=coo.shape)
    sorted_again = lineages.extend_strain_lineages(loaded, strain_of, qnames, strain_of_query, qr, qq, rnames)
    rows = lineages._stored_rows(loaded["a"], 12)
    d_s = min(loaded["a"].max_search_depth, 11)
    assert (np.diff(rows[1].reshape(12, d_s), axis=1) >= 0).all()
    assert sorted(sorted_again["a"][0].nn_dists.data.tolist()) == sorted(got["a"][0].nn_dists.data.tolist())


def test_errors(on_model):
    rr, qr, qq, rnames, qnames, strain_of, strain_of_query = make_case()
    fitted = {s: e[0] for s, e in lineages.fit_strain_lineages(rr, rnames, strain_of, [1, 2], min_count=10).items()}
    other = lineages.fit_strain_lineages(rr, rnames, {"c": strain_of["c"]}, [1, 3], min_count=10)["c"][0]
    with pytest.raises(RuntimeError, match="the lineage models of strains a and c differ in ranks, search depth or flags"):
        lineages.extend_strain_lineages(dict(fitted, c=other), strain_of, qnames, strain_of_query, qr, qq, rnames)
    with pytest.raises(RuntimeError, match="Trying to extend an unfitted model"):
        lineages.extend_strain_lineages(dict(fitted, a=models.LineageRanks([1, 2], 10000)), strain_of, qnames,
                                        strain_of_query, qr, qq, rnames)
    with pytest.raises(RuntimeError, match="does not hold the 840 pairs of 14 queries and 60 references"):
        lineages.extend_strain_lineages(fitted, strain_of, qnames, strain_of_query, qr[:-1], qq, rnames)
    with pytest.raises(RuntimeError, match="does not hold the 91 pairs of 14 queries"):
        lineages.extend_strain_lineages(fitted, strain_of, qnames, strain_of_query, qr, qq[:-1], rnames)
    with pytest.raises(RuntimeError, match="a lineage model of 12 samples for a strain of 11 members"):
        lineages.extend_strain_lineages(fitted, dict(strain_of, a=strain_of["a"][:-1]), qnames, strain_of_query, qr,
                                        qq, rnames)
    # no query in a strain with a model: nothing to do, and no device is asked
    assert lineages.extend_strain_lineages(fitted, strain_of, qnames, {qnames[1]: "x"}, qr, qq, rnames) == {}
    # a row of another length is not in the device's layout
    coo = fitted["a"].nn_dists
    from scipy.sparse import coo_matrix
    short = models.LineageRanks([1, 2], 10000)
    short.nn_dists = coo_matrix((coo.data[1:], (coo.row[1:], coo.col[1:])), shape=coo.shape)
    assert lineages._stored_rows(short, 12) is None


@pytest.mark.parametrize("run", ["default", "flags"])
def test_golden_case_on_the_model(run, tmp_path, capsys, on_model, monkeypatch):
    """--query-db and extend_strain_lineages on the recorded case: the reference's files, arrays and dicts."""
    import lineage_query_golden
    lineage_query_golden.run_and_check(tmp_path, run, capsys, monkeypatch)


def test_golden_case_has_the_properties_it_was_chosen_for():
    import lineage_query_golden
    texts, arrays = lineage_query_golden.load()
    qr, qq, template = arrays["qr"], arrays["qq"], arrays["template"]
    n_ref = len(qr) // 30
    assert all(qr[q * n_ref + template[q], 0] == 0 for q in range(4))                # copies of a reference
    assert qq[4 * (2 * 30 - 4 - 1) // 2 + 0, 0] == 0 and np.array_equal(qr[4 * n_ref:5 * n_ref], qr[5 * n_ref:6 * n_ref])
    placed = texts["strain_of_query"]
    for run in ("default", "flags"):
        strains = texts["runs"][run]["strains"]
        assert placed["queries/q06.fa"] not in strains and placed["queries/q07.fa"] not in strains
        assert sum(len(s["qNames"]) for s in strains.values()) == 28
        # a cross-side run of equal distances: a copy's row holds the floor for its reference, and the reference's row
        # holds it for the copy, in front of everything stored
        s = placed["queries/q00.fa"]
        data = arrays["%s_%s_nn_data" % (run, s)]
        assert (data == np.float32(1e-10)).sum() >= 2


def test_query_db_messages_and_exits(tmp_path, capsys, monkeypatch):
    import pickle
    scheme = ["refdb", [], "refdb", "refdb/refdb_clusters.csv", "Cluster", "refdb/refdb.dists", [13], 16, False, 10000,
              [1, 2], False, 10, False, False, False, False, False, {"1": "strain_1_lineage_db"}]
    path = str(tmp_path / "scheme.pkl")
    with open(path, "wb") as f:
        pickle.dump(scheme, f)
    with pytest.raises(SystemExit) as e:
        lineages.main(["--query-db", "q", "--db-scheme", path, "--output", "refdb"])
    assert e.value.code == 1
    assert capsys.readouterr().err == "--output and --ref-db must be different to prevent overwrite.\n"
    args = lineages.get_options(["--query-db", "q", "--db-scheme", path, "--output", "x"])
    args.output = None
    with pytest.raises(SystemExit):
        lineages.query_db(args)
    assert capsys.readouterr().err == "Need an output file name\n"
    with pytest.raises(SystemExit):
        lineages.get_options(["--query-db", "q", "--create-db", "db", "--db-scheme", path, "--output", "x"])
    capsys.readouterr()
    # no strain with a lineage database receives a query
    from poppunk_amd import sketchdb
    os.makedirs(tmp_path / "refdb")
    with open(tmp_path / "refdb" / "refdb.dists.pkl", "wb") as f:
        pickle.dump([["r0", "r1"], ["r0", "r1"], True], f)
    sketchdb.save_npz(str(tmp_path / "q" / "q"), ["a"], [13], np.zeros((1, 1, 2), dtype=np.uint64), 2, 14)
    monkeypatch.setattr(lineages, "_query_distances", lambda *a, **kw: (np.zeros((2, 2), dtype=np.float32),
                                                                       np.zeros((0, 2), dtype=np.float32)))
    monkeypatch.setattr(lineages, "_assign_strains", lambda *a, **kw: {"combined": {"r0": "1", "r1": "1", "a": "7"}})
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with pytest.raises(RuntimeError, match="no strain with a lineage database received a query"):
            lineages.main(["--query-db", "q", "--db-scheme", path, "--output", "out"])
    finally:
        os.chdir(cwd)


def test_abi_entries_and_argument_errors():
    lib = _lib.lib()
    for name in ("ppk_strain_extend_dev", "ppk_strain_extend"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    llp = C.POINTER(C.c_longlong)
    one = np.zeros(8, dtype=np.int64)
    onef = np.zeros(8, dtype=np.float32)

    def extend(seg, qoff, n_ref=10, n_qry=4, col=0, depth=3, qq=onef):
        seg, qoff = np.asarray(seg, dtype=np.int64), np.asarray(qoff, dtype=np.int64)
        rc = lib.ppk_strain_extend_dev(one.ctypes.data, seg.ctypes.data_as(llp), one.ctypes.data, qoff.ctypes.data_as(llp),
                                       len(seg) - 1, one.ctypes.data, onef.ctypes.data, onef.ctypes.data,
                                       None if qq is None else qq.ctypes.data, n_ref, n_qry, col, 1e-10, depth,
                                       one.ctypes.data, one.ctypes.data, onef.ctypes.data, None)
        return rc, _lib.last_error()
    assert extend([0, 2, 3], [0, 1, 1]) == (_lib.ERR_ARG, "ppk_strain_extend: strain 1 has 1 members: a strain needs at least 2")
    assert extend([0, 2, 5], [1, 1, 1]) == (_lib.ERR_ARG, "ppk_strain_extend: qry_off[0] must be 0")
    assert extend([0, 2, 5], [0, 2, 1]) == (_lib.ERR_ARG, "ppk_strain_extend: strain 1 has a negative number of queries")
    assert extend([0, 2, 5], [0, 1, 3], qq=None) == (_lib.ERR_ARG, "ppk_strain_extend: strain 1 has 2 queries and d_qq is NULL")
    assert extend([0, 2, 5], [0, 1, 1], col=2) == (_lib.ERR_ARG, "ppk_strain_extend: dist_col must be 0 or 1")
    assert extend([0, 2, 5], [0, 1, 1], depth=0) == (_lib.ERR_ARG, "ppk_strain_extend: depth must be at least 1")
    assert extend([0, 2, 5], [0, 1, 1], n_ref=1) == (_lib.ERR_ARG, "ppk_strain_extend: n_ref must be 2 .. 2^31 - 2")


def test_query_rows_are_indexed_in_64_bits():
    """q * n_ref + r on a database of 100 000 references and 30 000 queries: the last row is 2 999 999 999."""
    assert engine.qr_row_index(29999, 99999, 100000) == 2999999999
    assert engine.qr_row_index(np.int32(29999), np.int32(99999), np.int32(100000)) == 2999999999
