"""CPU tests of the silhouette's host side: the numpy restatement of the rule
(tests/silhouette_model.py) against sklearn's recorded arrays within the derived bound, the shift rule, the label
factorisation and sklearn's errors, the script's CSV rules on files of its formats (the device call replaced by the
restatement), and the argument errors that must come back without a device."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import silhouette_model as model
from poppunk_amd import _lib, engine, scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "silhouette.npz"))


def test_model_against_sklearn_within_the_bound(golden):
    assert str(golden["sklearn_version"]) == "1.7.2"
    tiny = zeros = 0
    for k in range(int(golden["n_cases"])):
        x, labels = golden["case%d_x" % k], golden["case%d_labels" % k]
        n = len(labels)
        for metric in range(4):
            sk, a_ref, b_ref = (golden["case%d_%s%d" % (k, what, metric)] for what in ("sk", "a", "b"))
            a, b, s, n_labels, valid = model.silhouette(x, labels, metric)
            eps, allowed = model.bound(x, metric, n, a_ref, b_ref)
            assert valid[0] == 1 and n_labels[0] == len(np.unique(labels))
            assert np.abs(a[0] - a_ref).max() <= eps and np.abs(b[0] - b_ref).max() <= eps, (k, metric)
            worst = np.abs(s[0] - sk)
            assert np.all(worst <= allowed), (k, metric, float(worst.max()))
            assert np.all(s[0][np.maximum(a_ref, b_ref) == 0] == 0)
            if n > 5:       # the bound bites: most samples have a denominator of ordinary size
                assert np.mean(np.maximum(a_ref, b_ref) >= 1e-6) >= 0.9, (k, metric)
            d = model.metric_f32(x, metric)
            tiny += int(np.sum((d > 0) & (d < 2.0 ** -17)))
            zeros += int(np.sum(d == 0))
    assert tiny > 1000 and zeros > 100      # the fixed point is exercised: values that are no multiple of 2^-40


def test_shift_rule():
    assert engine.silhouette_shift(3) == 40 and engine.silhouette_shift(1 << 21) == 40
    assert engine.silhouette_shift((1 << 21) + 1) == 39
    assert engine.silhouette_shift(100_000) == 40 and engine.silhouette_shift(10_000_000) == 61 - 24
    for n in (3, 5, 64, 65, 130, 257, 1 << 21, (1 << 21) + 1, 1 << 30):
        assert engine.silhouette_shift(n) == model.shift_of(n)
        # n distances of at most sqrt 2 stay below 2^62
        assert n * (int(np.sqrt(2.0) * 2.0 ** engine.silhouette_shift(n)) + 1) < 1 << 62


def test_factorise_and_label_count_errors():
    numbers, count = scores.factorise(["b", "a", "b", ("t", 1), 7, "a", 7.0])
    assert numbers.dtype == np.int32 and numbers.tolist() == [1, 2, 1, 3, 4, 2, 4] and count == 4
    x = np.zeros((6, 2), dtype=np.float32)      # n = 4
    with pytest.raises(ValueError, match=re.escape("Number of labels is 1. Valid values are 2 to n_samples - 1 "
                                                   "(inclusive)")):
        scores.silhouette_samples(x, ["a"] * 4)
    with pytest.raises(ValueError, match=re.escape("Number of labels is 4. Valid values are 2 to n_samples - 1 "
                                                   "(inclusive)")):
        scores.silhouette_score(x, list("abcd"))
    with pytest.raises(ValueError, match="inconsistent numbers of samples"):
        scores.silhouette_samples(x, ["a", "b", "a"])
    with pytest.raises(ValueError, match="metric must be one of"):
        scores.silhouette_samples(x, list("aabb"), metric="cosine")
    with pytest.raises(ValueError, match=r"n\(n-1\)/2"):
        scores.silhouette_samples(np.zeros((5, 2), dtype=np.float32), list("aabb"))
    assert scores.METRICS == {"core": 0, "accessory": 1, "euclidean": 2, "difference": 3}


def model_call(distMat, levels, metric, device_id=0):
    _, _, s, n_labels, valid = model.silhouette(np.asarray(distMat), levels, metric)
    return s, n_labels, valid


def test_scores_against_the_model(golden, monkeypatch):
    monkeypatch.setattr(scores, "_device_silhouette", model_call)
    x, labels = golden["case2_x"], golden["case2_labels"]
    names = ["cluster_%d" % c for c in labels]
    for name, code in scores.METRICS.items():
        want = model.silhouette(x, scores.factorise(names)[0], code)[2][0]
        assert np.array_equal(scores.silhouette_samples(x, names, metric=name), want)
        assert scores.silhouette_score(x, names, metric=name) == float(np.mean(want))
        # the numbers a clustering carries do not matter, only which samples share one
        assert np.array_equal(want, model.silhouette(x, labels, code)[2][0])


def write_case(tmp_path, golden, is_self=True, suffix=""):
    x, labels = golden["case3_x"], golden["case3_labels"]      # n = 5
    names = ["s%d%s" % (k, suffix) for k in range(5)]
    prefix = str(tmp_path / "db.dists")
    with open(prefix + ".pkl", "wb") as f:
        pickle.dump([names, names, is_self], f)
    np.save(prefix + ".npy", x)
    return prefix, x, labels, names


def test_calculate_silhouette_csv_columns_sub_and_errors(golden, tmp_path, monkeypatch):
    monkeypatch.setattr(scores, "_device_silhouette", model_call)
    prefix, x, labels, names = write_case(tmp_path, golden, suffix=".fa")
    want = float(np.mean(model.silhouette(x, labels, 2)[2][0]))
    other = [1, 2, 1, 2, 1]                                      # another clustering, in another column
    want_other = float(np.mean(model.silhouette(x, other, 2)[2][0]))
    assert want != want_other
    # the script's defaults: ids in column 1, clusters in column 2; rows in any order, quoted fields
    csv1 = str(tmp_path / "c1.csv")
    with open(csv1, "w") as f:
        f.write("Taxon,Cluster,Other\n")
        for k in (3, 0, 4, 1, 2):
            f.write('"%s",%d,%d\n' % (names[k], labels[k], other[k]))
    assert scores.calculate_silhouette(prefix, csv1) == want
    assert scores.calculate_silhouette(prefix, csv1, cluster_col=3) == want_other
    assert scores.calculate_silhouette(prefix, csv1, metric="core") == float(np.mean(model.silhouette(x, labels, 0)[2][0]))
    # ids in column 2: the cluster column counts among the REMAINING columns, so cluster_col = 2 is the file's first
    csv2 = str(tmp_path / "c2.csv")
    with open(csv2, "w") as f:
        f.write("Cluster,Taxon,Other\n")
        for k in range(5):
            f.write("%d,%s,%d\n" % (labels[k], names[k], other[k]))
    assert scores.calculate_silhouette(prefix, csv2, id_col=2) == want
    assert scores.calculate_silhouette(prefix, csv2, id_col=2, cluster_col=3) == want_other
    # sub is stripped from the names of both sides
    csv3 = str(tmp_path / "c3.csv")
    with open(csv3, "w") as f:
        f.write("Taxon,Cluster\n")
        for k in range(5):
            f.write("s%d.fasta,%d\n" % (k, labels[k]))
    with pytest.raises(KeyError):
        scores.calculate_silhouette(prefix, csv3)
    assert scores.calculate_silhouette(prefix, csv3, sub=r"\.fa(sta)?$") == want
    # the module's command line prints the score
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with redirect_stdout(buf):
        scores.main(["--distances", prefix, "--cluster-csv", csv2, "--id-col", "2", "--metric", "euclidean"])
    assert float(buf.getvalue()) == want
    # a query-vs-reference database is refused in the script's words
    sub = tmp_path / "qr"
    sub.mkdir()
    prefix_qr, _, _, _ = write_case(sub, golden, is_self=False)
    with pytest.raises(RuntimeError, match="Distance DB should be self-self distances"):
        scores.calculate_silhouette(prefix_qr, csv1)


def test_symbols_and_options_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppk.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("ppk_silhouette_dev", "ppk_silhouette"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    for name, default in (("silhouette_band", 0), ("silhouette_window", 0)):
        if "PPK_" + name.upper() not in os.environ:
            assert _lib.get_option(name) == default
    assert _lib.get_option("silhouette_scratch_mb") > 0
    assert callable(engine.silhouette_dev) and callable(scores.silhouette_of_levels)


def test_argument_errors_come_back_without_a_device():
    lib = _lib.lib()
    fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    d = np.zeros((10, 2), dtype=np.float32)
    lab = np.ones(8, dtype=np.int32)
    s = np.zeros(8, dtype=np.float64)
    w = np.zeros(2, dtype=np.int32)

    def call(n_rows=6, metric=2, n_levels=1, shift=40, dist=d, labels=lab):
        rc = lib.ppk_silhouette(dist.ctypes.data_as(fp) if dist is not None else None, n_rows, metric,
                                labels.ctypes.data_as(ip) if labels is not None else None, n_levels, shift, 0, None,
                                None, s.ctypes.data_as(dp), w.ctypes.data_as(ip), w.ctypes.data_as(ip))
        return rc, _lib.last_error()

    assert call(n_rows=5) == (_lib.ERR_ARG, "ppk_silhouette: row count is not n(n-1)/2 for any n (self/condensed "
                                            "matrix expected)")
    assert call(n_rows=1) == (_lib.ERR_ARG, "ppk_silhouette: n must be at least 3")
    assert call(n_rows=0) == (_lib.ERR_ARG, "ppk_silhouette: n must be at least 3")
    for metric in (-1, 4):
        assert call(metric=metric) == (_lib.ERR_ARG, "ppk_silhouette: metric must be 0 .. 3")
    for shift in (-1, 41):
        assert call(shift=shift) == (_lib.ERR_ARG, "ppk_silhouette: shift must be 0 .. 40")
    for n_levels in (0, 1024):
        assert call(n_levels=n_levels) == (_lib.ERR_ARG, "ppk_silhouette: n_levels must be 1 .. 1023")
    assert call(dist=None) == (_lib.ERR_ARG, "ppk_silhouette: NULL array")
    assert call(labels=None) == (_lib.ERR_ARG, "ppk_silhouette: NULL array")
    # above the rule: 2^21 + 1 samples allow 39 (the rows are never read: the check comes first)
    n = (1 << 21) + 1
    rc, err = call(n_rows=n * (n - 1) // 2, shift=40)
    assert rc == _lib.ERR_ARG and err.startswith("ppk_silhouette: shift must be at most 61 - ceil_log2(n)")
    # the device form refuses the same arguments before it asks for a device
    rc = lib.ppk_silhouette_dev(C.c_void_p(8), 6, 7, C.c_void_p(8), 1, 40, None, None, C.c_void_p(8), C.c_void_p(8),
                                C.c_void_p(8), None)
    assert rc == _lib.ERR_ARG and _lib.last_error() == "ppk_silhouette: metric must be 0 .. 3"
    rc = lib.ppk_silhouette_dev(None, 6, 2, C.c_void_p(8), 1, 40, None, None, C.c_void_p(8), C.c_void_p(8),
                                C.c_void_p(8), None)
    assert rc == _lib.ERR_ARG and _lib.last_error() == "ppk_silhouette: NULL array"
