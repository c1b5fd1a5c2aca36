"""Host tests of the lineages within every strain, no GPU: the numpy restatement
(tests/lineage_model.py) against hand-worked cases; poppunk_amd.lineages' CSV, pickle, message and error logic with the
restatement standing in for the device; models.LineageRanks.save / load; the ABI entries and options."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import lineage_model as model
from poppunk_amd import _lib, lineages, models


def model_fit(dist, n, members, seg_off, depth, col, ranks, reciprocal_only, count_unique_distances, epsilon,
              device_id=0):
    """lineages._device_fit's contract, computed by the restatement."""
    lists = model.strain_knn(np.asarray(dist), n, members, seg_off, depth, col)
    _, _, numbers, outputs = model.strain_ranks(lists, seg_off, depth, ranks, reciprocal_only, count_unique_distances,
                                                epsilon)
    sizes = np.diff(seg_off)
    return lineages._split(lists, sizes * np.minimum(depth, sizes - 1)), outputs, numbers


@pytest.fixture
def on_model(monkeypatch):
    monkeypatch.setattr(lineages, "_device_fit", model_fit)


def test_model_on_a_hand_worked_strain():
    """Four samples on a line at 0, 1, 3, 7 (distances |a - b| / 8), local order (3, 0, 2, 1) -> positions 7, 0, 3, 1,
    and a fifth sample in no strain."""
    x = np.asarray([0.0, 1.0, 3.0, 7.0, 5.0]) / 8
    iu = np.triu_indices(5, 1)
    dist = np.stack([np.abs(x[iu[0]] - x[iu[1]])] * 2, axis=1).astype(np.float32)
    members, seg_off = np.asarray([3, 0, 2, 1], dtype=np.int64), np.asarray([0, 4], dtype=np.int64)
    i, j, d = model.strain_knn(dist, 5, members, seg_off, 10, 0)
    assert i.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert j.tolist() == [2, 3, 1, 3, 2, 0, 3, 1, 0, 1, 2, 0]       # local rows: 7 -> 3, 1, 0; 0 -> 1, 3, 7; ...
    assert (d * 8).tolist() == [4, 6, 7, 1, 3, 7, 2, 3, 4, 1, 2, 6]
    prefix, stream, numbers, outputs = model.strain_ranks((i, j, d), seg_off, 10, [1, 2])
    assert prefix.tolist() == [[2] * 4, [3] * 4]                    # kNN + 1 entries, as the reference keeps
    prefix, stream, numbers, outputs = model.strain_ranks((i, j, d), seg_off, 10, [1, 2], reciprocal_only=True)
    # rank 1 keeps 0 -> {2, 3}, 1 -> {3, 2}, 2 -> {3, 1}, 3 -> {1, 2}: reciprocal pairs (1, 2), (1, 3), (2, 3)
    assert stream.tolist() == [[0, 1, 1], [0, 2, 1], [0, 3, 1], [1, 2, 0], [1, 3, 0], [2, 3, 0]]
    assert numbers.tolist() == [[2, 1, 1, 1], [1, 1, 1, 1]]
    assert model.print_clusters_numbers(np.asarray([0, 1, 1, 2, 3, 3])).tolist() == [4, 2, 2, 3, 1, 1]


def make_db(tmp_path, n=40, seed=2):
    """A database directory with a stored matrix, a clusters CSV whose row order is not the database's, a strain below
    min_count (3 members), one of exactly min_count (5) and names that need isolateNameToLabel."""
    rng = np.random.default_rng(seed)
    names = ["dir/s%02d.fa" % k for k in range(n)]
    rows = n * (n - 1) // 2
    X = rng.random((rows, 2)).astype(np.float32)
    X[:, 0] = np.floor(X[:, 0] * 32) / 32
    db = str(tmp_path / "db")
    os.makedirs(db)
    with open(os.path.join(db, "db.dists.pkl"), "wb") as f:
        pickle.dump([names, names, True], f)
    np.save(os.path.join(db, "db.dists.npy"), X)
    np.savez(os.path.join(db, "db.npz"), kmers=np.asarray([13, 17, 21]), sketchsize64=16)
    order = rng.permutation(n)
    strain = {k: ("10" if k % 8 == 0 else "2" if k % 8 == 1 and k < 24 else "9") for k in range(n)}
    with open(os.path.join(db, "db_clusters.csv"), "w") as f:
        f.write("Taxon,Cluster\n")
        for k in order:
            f.write("%s,%s\n" % (names[k], strain[k]))
    return db, names, X, [names[k] for k in order], strain


def run_create(tmp_path, db, extra=()):
    os.chdir(tmp_path)
    argv = ["--create-db", db, "--db-scheme", str(tmp_path / "scheme.pkl"), "--output", str(tmp_path / "out")]
    lineages.main(argv + list(extra))


def test_create_db_files_and_messages(tmp_path, on_model, capsys):
    db, names, X, csv_order, strain = make_db(tmp_path)
    cwd = os.getcwd()
    try:
        run_create(tmp_path, db, ["--min-count", "5"])
        err = capsys.readouterr().err
        groups = {s: [nm for nm in csv_order if strain[int(nm[5:7])] == s] for s in ("10", "2", "9")}
        assert [len(groups[s]) for s in ("10", "2", "9")] == [5, 3, 32]
        # the fit of each kept strain, one at a time, through the same restatement
        want_rows, per_strain = [], {}
        for s in ("10", "9"):                                    # string order; "2" is below min_count
            got = lineages.fit_strain_lineages(X, names, {s: groups[s]}, [1, 2, 3], min_count=5)[s]
            per_strain[s] = got
            for nm in got[1][1]:                                 # rank 1's printClusters order
                want_rows.append(",".join([nm, s] + [str(got[1][r][nm]) for r in (1, 2, 3)] + [got[2]["overall"][nm]]))
        with open(tmp_path / "out.csv") as f:
            assert f.read() == "id,Cluster,Rank_1,Rank_2,Rank_3,overall\n" + "\n".join(want_rows) + "\n"
        lines = ["Identifying strains in existing database", "Extracting properties of database",
                 "Generating databases for individual strains"]
        for s in ("10", "2", "9"):
            lines.append("Making database for strain " + s)
            if s != "2":
                lines += ["Network for rank %d has %d lineages" % (r, max(per_strain[s][1][r].values()))
                          for r in (1, 2, 3)]
                lines.append("Parsed data, now writing to CSV")
        assert err == "\n".join(lines) + "\n"
        assert not os.path.exists(tmp_path / "strain_2_lineage_db")
        for s in ("10", "9"):
            d = tmp_path / ("strain_%s_lineage_db" % s)
            stem = "strain_%s_lineage_db" % s
            with open(d / (stem + "_lineages.csv")) as f:
                text = f.read().splitlines()
            assert text[0] == "id,Rank_1_Lineage,Rank_2_Lineage,Rank_3_Lineage,overall_Lineage"
            ov = per_strain[s][2]
            assert text[1:] == [",".join([nm.split("/")[-1].replace(".", "_")] + [str(ov[c][nm]) for c in ov])
                                for nm in groups[s]]
            with open(d / (stem + ".dists.pkl"), "rb") as f:
                assert pickle.load(f) == [groups[s], groups[s], True]
            assert os.readlink(d / (stem + ".h5")) == os.path.relpath(os.path.join(db, "db.h5"), d)
            loaded = models.LineageRanks.load(str(d))
            assert loaded.ranks == [1, 2, 3] and loaded.max_search_depth == 10000
            for rank in (1, 2, 3):
                a, b = loaded.lower_rank_dists[rank], per_strain[s][0].lower_rank_dists[rank]
                assert np.array_equal(a.row, b.row) and np.array_equal(a.col, b.col) and np.array_equal(a.data, b.data)
            with open(d / (stem + "_fit.pkl"), "rb") as f:
                assert pickle.load(f) == [[[1, 2, 3], 10000, False, False, 0, 1e-10], "lineage"]
        with open(tmp_path / "scheme.pkl", "rb") as f:
            scheme = pickle.load(f)
        assert len(scheme) == 19
        assert scheme[0] == db and scheme[1] == groups["9"] and scheme[2] == db
        assert scheme[3] == os.path.join(db, "db_clusters.csv") and scheme[4] == "Cluster"
        assert scheme[5] == os.path.join(db, "db.dists") and scheme[6].tolist() == [13, 17, 21] and scheme[7] == 16
        assert scheme[8:18] == [False, 10000, [1, 2, 3], False, 5, False, False, False, False, False]
        assert scheme[18] == {"10": "strain_10_lineage_db", "9": "strain_9_lineage_db"}

        # the --overwrite checks
        with pytest.raises(SystemExit) as e:
            run_create(tmp_path, db, ["--min-count", "5"])
        assert e.value.code == 1
        assert capsys.readouterr().err == "Output file %s exists; use --overwrite to replace it\n" % (tmp_path / "out.csv")
        os.remove(tmp_path / "out.csv")
        with pytest.raises(SystemExit):
            run_create(tmp_path, db, ["--min-count", "5"])
        assert capsys.readouterr().err == "Output file %s exists; use --overwrite to replace it\n" % (tmp_path / "scheme.pkl")
        run_create(tmp_path, db, ["--min-count", "5", "--overwrite", "--reciprocal-only", "--count-unique-distances",
                                  "--use-accessory", "--ranks", "1,2,4", "--max-search-depth", "8"])
        assert "--overwrite means {strain_db_name} will be deleted now\n" in capsys.readouterr().err
        with open(tmp_path / "out.csv") as f:
            assert f.readline() == "id,Cluster,Rank_1,Rank_2,Rank_4,overall\n"
        with open(tmp_path / "strain_9_lineage_db" / "strain_9_lineage_db_fit.pkl", "rb") as f:
            assert pickle.load(f) == [[[1, 2, 4], 9, True, True, 1, 1e-10], "lineage"]
    finally:
        os.chdir(cwd)


def test_create_db_errors(tmp_path, on_model, capsys):
    db, names, X, csv_order, strain = make_db(tmp_path)
    cwd = os.getcwd()
    try:
        with pytest.raises(SystemExit) as e:
            run_create(tmp_path, db, ["--ranks", "1,2,3", "--max-search-depth", "3"])
        assert e.value.code == 1
        assert capsys.readouterr().err.endswith("Max search depth must be greater than the highest lineage rank\n")
        # strain "10" has 5 members: rank 5 is not below that, and nothing is written
        with pytest.raises(RuntimeError, match="Maximum rank must be less than the number of samples: 5"):
            run_create(tmp_path, db, ["--min-count", "5", "--ranks", "1,5"])
        assert not os.path.exists(tmp_path / "out.csv") and not os.path.exists(tmp_path / "strain_10_lineage_db")
        with pytest.raises(SystemExit):
            run_create(tmp_path, db, ["--query-db", "q.txt"])      # exclusive with --create-db
    finally:
        os.chdir(cwd)


def test_lineage_ranks_save_and_load(tmp_path, on_model):
    db, names, X, csv_order, strain = make_db(tmp_path)
    got = lineages.fit_strain_lineages(X, names, {"a": names[:12]}, [2, 1], max_search_depth=4,
                                       count_unique_distances=True, use_accessory=True, min_count=1)["a"][0]
    prefix = str(tmp_path / "some_db")
    os.makedirs(prefix)
    got.save(prefix)
    assert sorted(os.listdir(prefix)) == ["some_db_fit.pkl", "some_db_rank_1_fit.npz", "some_db_rank_2_fit.npz",
                                          "some_db_sparse_dists.npz"]
    back = models.LineageRanks.load(prefix)
    assert (back.ranks, back.max_search_depth, back.reciprocal_only, back.count_unique_distances, back.dist_col,
            back.resolution) == ([1, 2], 7, False, True, 1, 1e-10)
    for a, b in [(back.nn_dists, got.nn_dists)] + [(back.lower_rank_dists[r], got.lower_rank_dists[r]) for r in (1, 2)]:
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32
        assert np.array_equal(a.row, b.row) and np.array_equal(a.col, b.col) and np.array_equal(a.data, b.data)
    assert got.nn_dists.data.min() >= np.float32(1e-10)
    with pytest.raises(RuntimeError, match="Trying to save unfitted model"):
        models.LineageRanks([1], 10).save(prefix)


def test_abi_entries_and_options():
    lib = _lib.lib()
    for name in ("ppk_strain_knn_dev", "ppk_strain_ranks_dev", "ppk_strain_knn", "ppk_strain_ranks"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    for name, default in (("lineage_scratch_mb", 1024), ("lineage_lds_keys", 0)):
        if "PPK_" + name.upper() not in os.environ:
            assert _lib.get_option(name) == default


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    llp, fp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    dist = np.zeros((10, 2), dtype=np.float32)
    members = np.arange(5, dtype=np.int64)
    out = np.zeros(32, dtype=np.int64)
    outf = np.zeros(32, dtype=np.float32)

    def knn(seg, n=5, col=0, depth=3):
        seg = np.asarray(seg, dtype=np.int64)
        rc = lib.ppk_strain_knn_dev(dist.ctypes.data, n, col, members.ctypes.data, seg.ctypes.data_as(llp), len(seg) - 1,
                                    depth, out.ctypes.data, out.ctypes.data, outf.ctypes.data, None)
        return rc, _lib.last_error()
    assert knn([0, 2, 3, 5]) == (_lib.ERR_ARG, "ppk_strain_knn: strain 1 has 1 members: a strain needs at least 2")
    assert knn([1, 3, 5]) == (_lib.ERR_ARG, "ppk_strain_knn: seg_off[0] must be 0")
    assert knn([0, 2, 5], col=2) == (_lib.ERR_ARG, "ppk_strain_knn: dist_col must be 0 or 1")
    assert knn([0, 2, 5], depth=0) == (_lib.ERR_ARG, "ppk_strain_knn: depth must be at least 1")
    assert knn([0, 2, 5], n=1) == (_lib.ERR_ARG, "ppk_strain_knn: n must be 2 .. 2^31 - 2")
    seg = np.asarray([0, 2, 5], dtype=np.int64)
    n_out = C.c_size_t(7)

    def ranks(r):
        r = np.asarray(r, dtype=np.int32)
        rc = lib.ppk_strain_ranks_dev(out.ctypes.data, outf.ctypes.data, seg.ctypes.data_as(llp), 2, 3,
                                      r.ctypes.data_as(ip), len(r), 0, 0, 1e-10, out.ctypes.data, out.ctypes.data,
                                      out.ctypes.data, out.ctypes.data, None, 32, C.byref(n_out), None)
        return rc, _lib.last_error()
    assert ranks([2, 1]) == (_lib.ERR_ARG, "ppk_strain_ranks: ranks must be at least 1 and ascending")
    assert ranks([0]) == (_lib.ERR_ARG, "ppk_strain_ranks: ranks must be at least 1 and ascending")
    assert n_out.value == 0


def test_golden_case_has_the_properties_it_was_chosen_for():
    import lineage_golden
    texts, arrays = lineage_golden.load()
    sizes = np.bincount(arrays["strain_numbers"])
    assert texts["min_count"] in sizes and (sizes[sizes > 0] < texts["min_count"]).any()
    assert not np.array_equal(arrays["csv_order"], np.arange(300))
    dist = arrays["dist"]
    assert (dist == 0).any() and len(np.unique(dist[:, 0])) < 300
    assert set(texts["runs"]) == {"default", "flags"} and len(texts["runs"]["default"]["scheme"]) == 19


@pytest.mark.parametrize("run", ["default", "flags"])
def test_model_and_create_db_against_the_reference_python(run, tmp_path, on_model, capsys):
    """The restatement (through lineages.create_db, in the device's place) gives the arrays and files the reference's
    own Python wrote."""
    import lineage_golden
    lineage_golden.run_and_check(tmp_path, run, capsys)
