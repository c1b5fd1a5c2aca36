"""CPU tests of the Rand indices' host side: every Python score, computed from the numpy restatement
of the device's sums (tests/contingency_model.py), against the floats recorded from sklearn 1.7.2 and from the
reference script with ==; calculate_rand_indices on the recorded CSVs (the device call replaced by the restatement)
against the script's recorded output byte for byte, its messages and its exit code; the two symbols and the options;
the argument errors that must come back without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contingency_model as model
from poppunk_amd import _lib, engine, rand_indices, scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "rand.npz"))


@pytest.fixture
def on_model(monkeypatch):
    monkeypatch.setattr(scores, "_device_sums", model.device_call)


def test_model_on_a_table_worked_by_hand():
    # a: {0 1 2} {3 4} {5}; b: {0 1} {2 3} {4 5}: cells 2 1 | 1 1 | 1
    a, b = np.array([1, 1, 1, 2, 2, 6]), np.array([4, 4, 2, 2, 3, 3])
    sq_a, sq_b, labels_a, labels_b, sq_cells, n_cells = model.contingency_sums(a, b)
    assert (sq_a.tolist(), sq_b.tolist(), labels_a.tolist(), labels_b.tolist()) == ([14], [12], [3], [3])
    assert sq_cells.tolist() == [[8]] and n_cells.tolist() == [[5]]
    both = model.contingency_sums(np.stack([a, b]))
    assert both[4].tolist() == [[14, 8], [8, 12]] and both[5].tolist() == [[3, 5], [5, 3]]
    assert both[0].dtype == np.int64 and both[2].dtype == np.int32 and both[5].dtype == np.int64


def test_scores_equal_the_recorded_sklearn_and_script_floats(golden, on_model):
    assert str(golden["sklearn_version"]) == "1.7.2"
    assert int(golden["n_pairs"]) >= 12
    below_zero = ones = 0
    for k in range(int(golden["n_pairs"])):
        t, p = golden["pair%d_true" % k], golden["pair%d_pred" % k]
        for true, pred in ((t, p), (["c%d" % c for c in t], [("p", int(c)) for c in p])):   # any hashable names
            c = scores.pair_confusion_matrix(true, pred)
            assert c.dtype == np.int64 and np.array_equal(c, golden["pair%d_confusion" % k]), k
            assert scores.rand_score(true, pred) == float(golden["pair%d_rand" % k]), k
            assert scores.adjusted_rand_score(true, pred) == float(golden["pair%d_ari" % k]), k
            assert scores.rand_index_score(true, pred) == float(golden["pair%d_ri" % k]), k
        below_zero += float(golden["pair%d_ari" % k]) < 0
        ones += float(golden["pair%d_ri" % k]) == 1.0
    assert below_zero >= 1 and ones >= 3
    # argument order matters to the confusion matrix alone
    t, p = golden["pair5_true"], golden["pair5_pred"]
    assert np.array_equal(scores.pair_confusion_matrix(p, t), golden["pair5_confusion"].T)
    assert isinstance(scores.adjusted_rand_score(t, p), float) and isinstance(scores.rand_score(t, p), float)


def test_unequal_lengths_and_empty_labelings(on_model):
    with pytest.raises(ValueError, match=re.escape("Found input variables with inconsistent numbers of samples: "
                                                   "[3, 4]")):
        scores.adjusted_rand_score([1, 2, 3], [1, 2, 3, 4])
    with pytest.raises(ValueError, match="inconsistent numbers of samples"):
        scores.pair_confusion_matrix([1], [])
    assert scores.rand_score([], []) == 1.0 and scores.adjusted_rand_score([], []) == 1.0
    assert scores.rand_index_score([], []) == 1.0
    assert scores.pair_confusion_matrix([], []).tolist() == [[0, 0], [0, 0]]


def test_rand_of_levels_from_one_call(golden, monkeypatch):
    calls = []

    def counted(levels_a, levels_b=None, device_id=0):
        calls.append(1)
        return model.contingency_sums(levels_a, levels_b)

    monkeypatch.setattr(scores, "_device_sums", counted)
    fine = scores.factorise(golden["pair6_true"])[0]
    coarse = scores.factorise(golden["pair6_pred"])[0]
    other = scores.factorise(golden["pair7_pred"])[0]
    levels = np.stack([fine, coarse, other, np.ones_like(fine)])
    rand, adjusted, refines = scores.rand_of_levels(levels)
    assert len(calls) == 1
    assert rand.shape == adjusted.shape == refines.shape == (4, 4) and rand.dtype == adjusted.dtype == np.float64
    assert rand[0, 1] == rand[1, 0] == float(golden["pair6_rand"])
    assert adjusted[0, 1] == adjusted[1, 0] == float(golden["pair6_ari"])
    assert adjusted[0, 2] == 1.0 and np.all(np.diag(adjusted) == 1.0) and np.all(np.diag(rand) == 1.0)
    # fine and its renamed copy refine each other and everything coarser; nothing coarser refines them
    assert refines.tolist() == [[True, True, True, True], [False, True, False, True], [True, True, True, True],
                                [False, False, False, True]]
    r2, a2, f2 = scores.rand_of_levels(levels[:2], levels[2:])
    assert np.array_equal(r2, rand[:2, 2:]) and np.array_equal(a2, adjusted[:2, 2:])
    assert np.array_equal(f2, refines[:2, 2:])


def write_files(golden, where):
    for name, text in zip(golden["file_names"], golden["file_texts"]):
        with open(os.path.join(str(where), str(name)), "w") as f:
            f.write(str(text))


@pytest.mark.parametrize("run", ["same_names", "same_names_subset", "lacking_names", "misformatted_and_disjoint"])
def test_calculate_rand_indices_writes_the_script_s_bytes(golden, on_model, tmp_path, monkeypatch, capsys, run):
    assert run in golden["run_names"].tolist()
    write_files(golden, tmp_path)
    monkeypatch.chdir(tmp_path)
    inputs = [str(a) for a in golden[run + "_args"]]
    subset = str(golden[run + "_subset"]) or None
    assert int(golden[run + "_code"]) == 0
    rows = rand_indices.calculate_rand_indices(inputs, output="mine.out", subset=subset)
    assert open("mine.out").read() == str(golden[run + "_out"])
    assert capsys.readouterr().err == str(golden[run + "_err"])
    assert len(rows) == str(golden[run + "_out"]).count("\n") - 1
    # the command line, with the script's comma-separated list
    argv = ["--input", ",".join(inputs), "--output", "cli.out"] + (["--subset", subset] if subset else [])
    assert rand_indices.main(argv) == 0
    assert open("cli.out").read() == str(golden[run + "_out"])
    assert capsys.readouterr().err == str(golden[run + "_err"])


def test_a_missing_file_ends_the_run_with_the_script_s_message_and_code(golden, on_model, tmp_path, monkeypatch, capsys):
    write_files(golden, tmp_path)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        rand_indices.main(["--input", ",".join(str(a) for a in golden["missing_file_args"]), "--output", "mine.out"])
    assert e.value.code == int(golden["missing_file_code"]) == 1
    assert capsys.readouterr().err == str(golden["missing_file_err"])
    assert not os.path.exists("mine.out") and str(golden["missing_file_out"]) == ""


def test_pairs_that_share_a_sample_set_share_a_device_call(golden, tmp_path, monkeypatch):
    shapes = []

    def counted(levels_a, levels_b=None, device_id=0):
        shapes.append((np.asarray(levels_a).shape, levels_b is None))
        return model.contingency_sums(levels_a, levels_b)

    monkeypatch.setattr(scores, "_device_sums", counted)
    write_files(golden, tmp_path)
    monkeypatch.chdir(tmp_path)
    rand_indices.calculate_rand_indices("a.csv,b.csv,d.csv", output="one.out")
    assert shapes == [((3, 40), True)]                      # three pairs, one call
    del shapes[:]
    rand_indices.calculate_rand_indices("a.csv,b.csv,c.csv", output="two.out")
    assert sorted(shapes) == [((2, 40), True), ((3, 29), True)]      # (a, b) on 40 names; (a, c) and (b, c) on c's 29


def test_item_errors_and_the_empty_cluster_field(on_model, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    open("x.csv", "w").write("Taxon,Cluster\ns1,1\ns2,1\ns1,2\ns3,2\n")      # s1 twice
    open("y.csv", "w").write("Taxon,Cluster\ns1,1\ns2,2\ns3,2\n")
    open("z.csv", "w").write("Taxon,Cluster\ns2,1\ns3,1\n")                  # lacks s1
    open("empty.csv", "w").write("Taxon,Cluster\ns1,1\ns2,\ns3,2\n")
    open("sub.txt", "w").write("s1\ns2\n")
    with pytest.raises(ValueError, match="can only convert an array of size 1 to a Python scalar"):
        rand_indices.calculate_rand_indices("x.csv,y.csv")                   # the first file holds a compared name twice
    # the second file holding it twice is no error in the script: the name is compared twice
    rows = rand_indices.calculate_rand_indices("y.csv,x.csv", output="dup.out")
    assert rows[0][:5] == ["y.csv", "x.csv", "3", "4", "4"]
    with pytest.raises(ValueError, match="can only convert an array of size 1"):
        rand_indices.calculate_rand_indices("y.csv,z.csv", subset="sub.txt")     # y has s1, z lacks it
    with pytest.raises(ValueError, match="can only convert an array of size 1"):
        rand_indices.calculate_rand_indices("y.csv,x.csv", subset="sub.txt")     # ... or holds it twice
    with pytest.raises(ValueError, match="empty.csv, line 3: empty Cluster field"):
        rand_indices.calculate_rand_indices("y.csv,empty.csv")
    # "1" and "01" are two clusters here ([EXT]: pandas would merge them in an all-numeric column)
    open("lead.csv", "w").write("Taxon,Cluster\ns1,1\ns2,01\ns3,01\n")
    rows = rand_indices.calculate_rand_indices("y.csv,lead.csv", output="lead.out")
    assert rows[0][5:] == ["1.0", "1.0"]


def test_symbols_and_options_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppk.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("ppk_contingency_sums_dev", "ppk_contingency_sums"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 12
    for name, default in (("rand_batch", 0), ("rand_wave_max", 64), ("rand_window", 0), ("rand_scratch_mb", 1024)):
        if "PPK_" + name.upper() not in os.environ:
            assert _lib.get_option(name) == default
    assert callable(engine.contingency_sums_dev) and callable(scores.rand_of_levels)


def test_argument_errors_come_back_without_a_device():
    lib = _lib.lib()
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    lab = np.ones(8, dtype=np.int32)
    big = np.zeros(4, dtype=np.int64)
    small = np.zeros(4, dtype=np.int32)

    def call(a=lab, n_a=1, b=None, n_b=0, n=8, sq_a=big, sq_b=big, labels_a=small, labels_b=small, sq_cells=big,
             n_cells=big):
        def ptr(x, t):
            return None if x is None else x.ctypes.data_as(t)
        rc = lib.ppk_contingency_sums(ptr(a, ip), n_a, ptr(b, ip), n_b, n, 0, ptr(sq_a, lp), ptr(sq_b, lp),
                                      ptr(labels_a, ip), ptr(labels_b, ip), ptr(sq_cells, lp), ptr(n_cells, lp))
        return rc, _lib.last_error()

    null = (_lib.ERR_ARG, "ppk_contingency_sums: NULL array")
    for which in ("a", "sq_a", "labels_a", "sq_cells", "n_cells"):
        assert call(**{which: None}) == null, which
    assert call(b=lab, n_b=1, sq_b=None) == null and call(b=lab, n_b=1, labels_b=None) == null
    assert call(n=0) == (_lib.ERR_ARG, "ppk_contingency_sums: n must be at least 1")
    assert call(n=(1 << 31) - 1) == (_lib.ERR_ARG, "ppk_contingency_sums: n must be below 2^31 - 1")
    levels = (_lib.ERR_ARG, "ppk_contingency_sums: n_a and n_b must be 1 .. 1023")
    assert call(n_a=0) == levels and call(n_a=1024) == levels
    assert call(b=lab, n_b=0) == levels and call(b=lab, n_b=1024) == levels
    # the device form refuses the same arguments before it asks for a device
    p = C.c_void_p(8)
    rc = lib.ppk_contingency_sums_dev(p, 1024, None, 0, 8, p, None, p, None, p, p, None)
    assert (rc, _lib.last_error()) == levels
    rc = lib.ppk_contingency_sums_dev(p, 1, None, 0, 8, p, None, p, None, None, p, None)
    assert (rc, _lib.last_error()) == null
    rc = lib.ppk_contingency_sums_dev(p, 1, p, 1, 0, p, p, p, p, p, p, None)
    assert (rc, _lib.last_error()) == (_lib.ERR_ARG, "ppk_contingency_sums: n must be at least 1")
