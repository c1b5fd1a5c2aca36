"""CPU tests of the cluster-number mirrors: printClusters' naming rules and CSV from number arrays,
readIsolateTypeFromCsv, multi_refine's file-index rule, the iterate family, nesting, tree cut and the accumulation
from bucket sums to cluster means -- against tests/golden/clusters_csv.json and clusters.npz (the reference's own
functions, make_golden_clusters.py).  No device is touched."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest

from poppunk_amd import _lib, iterate, network, refine, utils

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "clusters_csv.json")) as _f:
    DOC = json.load(_f)
NAMING = {c["name"]: c for c in DOC["naming"]}


def golden():
    return np.load(os.path.join(HERE, "golden", "clusters.npz"))


def run_case(case, tmp_path, capsys):
    old = ext = None
    if case["old_csv"] is not None:
        old = str(tmp_path / "old.csv")
        open(old, "w").write(case["old_csv"])
    if case["ext_csv"] is not None:
        ext = str(tmp_path / "ext.csv")
        open(ext, "w").write(case["ext_csv"])
    capsys.readouterr()
    got = network.print_cluster_numbers(np.array(case["numbers"]), case["names"], outPrefix=str(tmp_path / "out"),
                                        oldClusterFile=old, externalClusterCSV=ext, printRef=case["printRef"],
                                        write_unwords=False)
    return got, capsys.readouterr().err


def blocks(rows):
    """the cluster names of a CSV's rows in block order, and the mapping"""
    order = [k for k, _ in itertools.groupby(r[1] for r in rows)]
    return order, {r[0]: r[1] for r in rows}


def test_fixture_covers_the_rules():
    assert set(NAMING) == {"no_old_file", "exact_match", "merge_two", "merge_three", "split",
                           "new_names_with_merged_ids", "print_ref_false", "no_old_file_no_ref", "external"}
    assert "1_2" in NAMING["merge_two"]["clustering"].values()
    assert "2_3_1" in NAMING["merge_three"]["clustering"].values()         # the old file's order, not numeric
    assert "split across multiple new clusters" in NAMING["split"]["stderr"]
    assert "7" in NAMING["new_names_with_merged_ids"]["clustering"].values()
    assert NAMING["no_old_file_no_ref"]["error"] is not None
    # equal sizes: the component of the higher lowest vertex gets the smaller number (singletons 9, 10, 11 -> 4, 5, 6
    # reversed)
    assert NAMING["no_old_file"]["numbers"][9:] == [6, 5, 4]


@pytest.mark.parametrize("name", ["no_old_file", "exact_match", "merge_two", "merge_three", "split",
                                  "new_names_with_merged_ids", "print_ref_false", "external"])
def test_naming_rules_match_the_reference(name, tmp_path, capsys):
    case = NAMING[name]
    (clustering, merged), err = run_case(case, tmp_path, capsys)
    assert clustering == case["clustering"]
    want_type = str if case["old_csv"] is not None else int
    assert all(type(v) is want_type for v in clustering.values())
    assert sorted(merged) == case["merged"]
    assert err == case["stderr"]
    rows = [line.split(",") for line in open(str(tmp_path / "out_clusters.csv")).read().splitlines()]
    assert rows[0] == ["Taxon", "Cluster"]
    got_order, got_map = blocks(rows[1:])
    want_order, want_map = blocks(case["csv_rows"])
    assert got_map == want_map and got_order == want_order
    # the rows of one new cluster follow rlist
    for number in set(case["numbers"]):
        members = [r[0] for r in rows[1:] if case["numbers"][case["names"].index(r[0])] == number]
        assert members == sorted(members, key=case["names"].index)
    assert not os.path.exists(str(tmp_path / "out_unword_clusters.csv"))


def test_print_ref_false_drops_the_old_names(tmp_path, capsys):
    case = NAMING["print_ref_false"]
    run_case(case, tmp_path, capsys)
    taxa = [line.split(",")[0] for line in open(str(tmp_path / "out_clusters.csv")).read().splitlines()[1:]]
    assert taxa and all(t in ("s09", "s10", "s11") for t in taxa)
    assert sorted(taxa) == sorted(r[0] for r in case["csv_rows"])


def test_first_runtime_error_is_kept():
    case = NAMING["no_old_file_no_ref"]
    with pytest.raises(RuntimeError) as e:
        network.print_cluster_numbers(np.array(case["numbers"]), case["names"], outPrefix="unused", printRef=False)
    assert str(e.value) == case["error"]
    with pytest.raises(RuntimeError) as e:          # printClusters raises it before it asks the device for anything
        network.printClusters((np.zeros((0, 2), dtype=np.int64), 3), ["a", "b", "c"], printRef=False)
    assert str(e.value) == case["error"]


def test_unword_names_are_declined_in_one_line(tmp_path, capsys):
    case = NAMING["no_old_file"]
    network.print_cluster_numbers(np.array(case["numbers"]), case["names"], outPrefix=str(tmp_path / "o"))
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "_unword_clusters.csv" in err
    assert os.listdir(str(tmp_path)) == ["o_clusters.csv"]


def test_external_clusters_table(tmp_path, capsys):
    case = NAMING["external"]
    run_case(case, tmp_path, capsys)
    got = [line.split(",") for line in open(str(tmp_path / "out_external_clusters.csv")).read().splitlines()]
    want = case["ext_csv_out"]
    assert got[0] == want[0] == ["sample", "MLST", "Serotype"]           # every column but the last
    norm = lambda rows: {r[0]: [";".join(sorted(x.split(";"))) for x in r[1:]] for r in rows[1:]}
    assert norm(got) == norm(want)
    assert any(";" in x for r in got[1:] for x in r[1:]) and any("NA" in r for r in got[1:])


@pytest.mark.parametrize("case", DOC["read_csv"], ids=[c["name"] for c in DOC["read_csv"]])
def test_read_isolate_type_from_csv(case, tmp_path):
    path = str(tmp_path / "in.csv")
    open(path, "w").write(case["text"])
    sets = utils.readIsolateTypeFromCsv(path, mode=case["mode"], return_dict=False)
    assert [[col, [[k, sorted(v)] for k, v in d.items()]] for col, d in sets.items()] == case["sets"]
    dicts = utils.readIsolateTypeFromCsv(path, mode=case["mode"], return_dict=True)
    assert [[col, [[k, v] for k, v in d.items()]] for col, d in dicts.items()] == case["dicts"]


def test_read_isolate_type_unknown_mode_exits(tmp_path, capsys):
    path = str(tmp_path / "in.csv")
    open(path, "w").write("a,b\n1,2\n")
    with pytest.raises(SystemExit):
        utils.readIsolateTypeFromCsv(path, mode="nonsense")
    assert "Unknown CSV reading mode: nonsense" in capsys.readouterr().err


def test_boundary_files_quirk_matches_grow_network():
    z = golden()
    net = np.load(os.path.join(HERE, "golden", "network_sweep.npz"))
    n = int(net["holes_n"])
    counts = z["holes_edge_counts"]
    assert (counts == 0).sum() >= 5 and counts[0] == 0          # offsets without edges, the first among them
    assert np.array_equal(counts, np.bincount(net["holes_idx"], minlength=counts.size))
    n_clusters = net["holes_stats"][:, 1]                       # components of every G_t (networkx)
    files = refine.boundary_files(counts, n_clusters, n)
    assert [k for k, _ in files] == z["holes_file_idx"].tolist()
    grown = np.flatnonzero(counts > 0)
    for (k, idx), row in zip(files, z["holes_numbers"]):
        assert idx == grown[grown >= k][0]                       # the NEXT graph with edges, not the one before
        assert row.max() == n_clusters[idx]


def test_boundary_files_by_hand():
    # 5 samples, 6 offsets; edges arrive at offsets 1 and 4.  Offset 0 takes the graph of offset 1; 2, 3 that of 4; 5
    # is after the last offset with edges: nothing
    assert refine.boundary_files([0, 3, 0, 0, 2, 0], [5, 4, 4, 4, 3, 3], 5) == [(0, 1), (1, 1), (2, 4), (3, 4), (4, 4)]
    # a graph with as many clusters as samples is not written, and its indices are not made up for later
    assert refine.boundary_files([1, 0, 2], [5, 5, 3], 5) == [(1, 2), (2, 2)]
    assert refine.boundary_files([0, 0], [4, 4], 4) == []


def test_multi_refine_declines_subsampling_before_the_device():
    with pytest.raises(NotImplementedError):
        refine.multi_refine(None, ["a"], [0, 0], [1, 1], [1, 1], 0.5, 5, "x", sample_size=10)


# ---- iterate ------------------------------------------------------------------------------------------------------
NAMES8 = ["s%d" % k for k in range(8)]
LEVELS8 = np.array([[1, 1, 2, 2, 3, 4, 5, 6],
                    [1, 1, 1, 1, 2, 2, 3, 4],
                    [1, 1, 1, 1, 1, 1, 2, 3]])


def test_family_nesting_and_cut_by_hand():
    iterate.check_nested(LEVELS8)
    family, where, order, everyone = iterate.family_of_levels(LEVELS8, NAMES8)
    assert family == {1: {"s0", "s1"}, 2: {"s2", "s3"}, 3: {"s0", "s1", "s2", "s3"}, 4: {"s4", "s5"},
                      5: {"s0", "s1", "s2", "s3", "s4", "s5"}}
    assert where == {1: (0, 1), 2: (0, 2), 3: (1, 1), 4: (1, 2), 5: (2, 1)}
    assert order == [5, 3, 1, 2, 4] and everyone == set(NAMES8)
    parents, leftover = iterate.nest_family(family, order, everyone)
    assert parents == {5: "root", 3: 5, 1: 3, 2: 3, 4: 5}
    assert leftover["root"] == {"s6", "s7"} and leftover[3] == set() and leftover[4] == {"s4", "s5"}
    nwk = iterate.family_newick(parents, leftover, order, NAMES8)
    assert re.sub(r":[0-9.]+", "", nwk) == "((((s0,s1)cluster1,(s2,s3)cluster2)cluster3,(s4,s5)cluster4)cluster5,s6,s7)root;\n"
    # lengths pi / max: 5 -> 1.0, 3 -> 0.5, 4 -> 0.2, 1 and 2 -> 0.1.  cutoff 0.3: from s0 climb 1 (0.1) -> 3 (0.5 >
    # cutoff): select 1; likewise 2; 4 is below and its parent 5 above: select 4
    pi = {5: 0.10, 3: 0.05, 4: 0.02, 1: 0.01, 2: 0.01}
    assert iterate.cut_tree(parents, leftover, pi, 0.3, NAMES8) == [1, 2, 4]
    # cutoff 0.6: 1 -> 3 (0.5, still below) -> 5 (1.0 above): select 3; from s4: 4 below, 5 above: select 4
    assert iterate.cut_tree(parents, leftover, pi, 0.6, NAMES8) == [3, 4]
    # cutoff 0.05: nothing is below it
    assert iterate.cut_tree(parents, leftover, pi, 0.05, NAMES8) == []


def test_is_nested_and_reading_files(tmp_path):
    d = {"root": {"a", "b", "c", "d"}, 1: {"a", "b", "c"}, 2: {"a", "b"}}
    assert iterate.is_nested(d, {"a"}, ["root", 1, 2]) == 2
    assert iterate.is_nested(d, {"a", "c"}, ["root", 1, 2]) == 1
    assert iterate.is_nested(d, {"e"}, ["root", 1, 2]) is None
    prefix = str(tmp_path / "db")
    for k, row in enumerate(LEVELS8):
        network.print_cluster_numbers(row, NAMES8, outPrefix="%s_boundary%d" % (prefix, k), write_unwords=False)
    got = list(iterate.read_next_cluster_file(prefix))
    assert [g[2] for g in got] == [0, 1, 2]
    assert got[0][1] == {1: {"s0", "s1"}, 2: {"s2", "s3"}} and len(got[0][0]) == 6
    assert list(got[1][1].keys()) == [1, 2]                   # file order: size descending
    assert np.array_equal(iterate.levels_of_files(prefix, NAMES8), LEVELS8)


def test_nesting_check_rejects_a_split():
    with pytest.raises(ValueError, match="not nested"):
        iterate.check_nested(np.array([[1, 1, 2], [1, 2, 2]]))
    iterate.check_nested(np.array([[1, 2, 3], [1, 1, 2], [1, 1, 2], [1, 1, 1]]))


def test_bucket_sums_to_cluster_means_by_hand():
    n = 8
    pairs = list(itertools.combinations(range(n), 2))
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 20, len(pairs)).astype(np.int64)
    bs = np.zeros((3, n + 1), dtype=np.int64)
    bc = np.zeros((3, n + 1), dtype=np.int64)
    for (i, j), v in zip(pairs, x):
        for t in range(3):
            if LEVELS8[t, i] == LEVELS8[t, j]:
                bs[t, LEVELS8[t, i]] += v
                bc[t, LEVELS8[t, i]] += 1
                break
    ts, tc = iterate.cluster_totals(LEVELS8, bs, bc)
    means = iterate.cluster_means(LEVELS8, bs, bc, 20)
    for t in range(3):
        for c in np.unique(LEVELS8[t]):
            inside = [k for k, (i, j) in enumerate(pairs) if LEVELS8[t, i] == c and LEVELS8[t, j] == c]
            size = int((LEVELS8[t] == c).sum())
            assert tc[t, c] == len(inside) == size * (size - 1) // 2
            assert ts[t, c] == x[inside].sum()
            if inside:
                assert means[t, c] == x[inside].sum() / 2.0**20 / len(inside)
            else:
                assert np.isnan(means[t, c])


def test_family_of_the_reference_from_its_level_matrix():
    z = golden()
    n = z["multi_numbers"].shape[1]
    names = ["s%d" % k for k in range(n)]
    iterate.check_nested(z["multi_numbers"])
    family, where, order, _ = iterate.family_of_levels(z["multi_numbers"], names)
    assert list(family.keys()) == z["iter_ids"].tolist()
    for c, row in zip(z["iter_ids"].tolist(), z["iter_members"]):
        assert family[c] == {names[v] for v in np.flatnonzero(row)}
    assert order == z["iter_sorted"].tolist()
    assert float(z["iter_allowance"]) < 1e-6


def test_pair_sum_shift_rule():
    from poppunk_amd import engine
    assert engine.pair_sum_shift(1) == 40 and engine.pair_sum_shift(1 << 22) == 40
    assert engine.pair_sum_shift((1 << 22) + 1) == 39
    assert engine.pair_sum_shift(49995000) == 62 - 26


def test_new_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppk.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("ppk_cluster_sweep_dev", "ppk_cluster_sweep", "ppk_cluster_pair_sums_dev", "ppk_cluster_pair_sums"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    # host-side argument errors come back as codes with a message, with no device in reach
    lib = _lib.lib()
    one = np.ones(1, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    assert lib.ppk_cluster_sweep(None, None, None, 0, 1, 0, 0, one.ctypes.data_as(ip),
                                 one.ctypes.data_as(ip)) == _lib.ERR_ARG
    assert b"ppk_cluster_sweep: n_off must be 1 .. 1023" in lib.ppk_last_error()
    s = np.zeros(8, dtype=np.int64)
    llp = C.POINTER(C.c_longlong)
    d = np.zeros((2, 2), dtype=np.float32)
    assert lib.ppk_cluster_pair_sums(d.ctypes.data_as(C.POINTER(C.c_float)), 2, 0, one.ctypes.data_as(ip), 1, 40, 0,
                                     s.ctypes.data_as(llp), s.ctypes.data_as(llp)) == _lib.ERR_ARG
    assert b"row count is not n(n-1)/2" in lib.ppk_last_error()
