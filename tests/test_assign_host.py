"""CPU tests of the query-assignment mirrors: network.addQueryToNetwork,
construct_network_from_assignments, qc.qcQueryAssignments and assign.assign_query_clusters over every case of
tests/golden/assign.json (the reference's own functions, make_golden_assign.py), with a numpy restatement of the two
device calls -- links_restated, extend_restated, which tests/test_gpu_assign.py holds the device to -- standing in for
the device, the oracle for generateTuples and the model.  No device is touched."""
import json
import os

import numpy as np
import pytest

from poppunk_amd import _lib, assign, network, poppunk_refine, qc

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "assign.json")) as _f:
    DOC = json.load(_f)
CASES = {c["name"]: c for c in DOC["cases"]}
N_REF = len(DOC["rNames"])


def arrays():
    return np.load(os.path.join(HERE, "golden", "assign.npz"))


# ---- the two device calls, restated ----------------------------------------------------------------------------------
def links_restated(i, j, label, n_qry, max_links):
    """ppk_query_links: per query its query-reference edge count, the number of distinct labels at their reference
    ends, and the max_links smallest of those, ascending, padded with -1"""
    i, j, label = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(label, dtype=np.int64)
    n_ref = label.size
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    cross = (lo < n_ref) & (hi >= n_ref)
    q, lab = hi[cross] - n_ref, label[lo[cross]]
    degree = np.bincount(q, minlength=n_qry).astype(np.int32)
    n_links = np.zeros(n_qry, dtype=np.int32)
    links = np.full((n_qry, max_links), -1, dtype=np.int32)
    for query in np.unique(q).tolist():
        mine = np.unique(lab[q == query])
        n_links[query] = mine.size
        links[query, :min(mine.size, max_links)] = mine[:max_links]
    return degree, n_links, links


def ranking_restated(n, i, j):
    """printClusters' numbers from scipy: components in the order of their lowest vertex, len - rankdata(sizes,
    'ordinal') (PopPUNK/network.py:1538-1545)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.stats import rankdata
    if n == 0:
        return np.zeros(0, dtype=np.int32), 0
    adj = coo_matrix((np.ones(len(i)), (np.asarray(i), np.asarray(j))), shape=(n, n))
    n_comp, comp = connected_components(adj, directed=False)
    firsts = np.full(n_comp, n, dtype=np.int64)
    np.minimum.at(firsts, comp, np.arange(n))
    order = np.argsort(firsts)                      # scipy numbers components by first appearance already; be explicit
    renumber = np.empty(n_comp, dtype=np.int64)
    renumber[order] = np.arange(n_comp)
    comp = renumber[comp]
    sizes = np.bincount(comp, minlength=n_comp)
    ranks = n_comp - rankdata(sizes, method='ordinal').astype(int)
    return (ranks[comp] + 1).astype(np.int32), n_comp


def extend_restated(i, j, label, n_qry):
    """ppk_cluster_extend: the ranking of (a star per label over the references + the new edges)"""
    label = np.asarray(label, dtype=np.int64)
    n_ref = label.size
    first = np.full(max(n_ref, 1), n_ref, dtype=np.int64)
    np.minimum.at(first, label, np.arange(n_ref))
    star_i, star_j = np.arange(n_ref, dtype=np.int64), first[label] if n_ref else np.zeros(0, dtype=np.int64)
    keep = star_i != star_j
    return ranking_restated(n_ref + n_qry, np.concatenate([star_i[keep], np.asarray(i, dtype=np.int64)]),
                            np.concatenate([star_j[keep], np.asarray(j, dtype=np.int64)]))


def labels_restated(G):
    e = np.asarray(G[0], dtype=np.int64).reshape(-1, 2)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = int(G[1])
    return connected_components(coo_matrix((np.ones(e.shape[0]), (e[:, 0], e[:, 1])), shape=(n, n)),
                                directed=False)[1].astype(np.int32)


def knn1_restated(qrDistMat, n_qry, n_ref, dist_col):
    m = np.asarray(qrDistMat)[:, dist_col].reshape(n_qry, n_ref).astype(np.float64)
    for q in range(min(n_qry, n_ref)):
        m[q, q] = np.inf                            # src/extend.cpp:271 skips column i of row i
    return np.argmin(m, axis=1).astype(np.int64)


class OracleModel:
    """make_golden_assign.py's model: the oracle's threshold, within_label -1"""
    type = 'refine'
    threshold = False
    within_label = -1

    def assign(self, X, slope=2):
        from oracle import oracle
        T = DOC["x_max"] / 2
        x_max, y_max = {2: (DOC["x_max"], DOC["y_max"]), 0: (T, 0.0), 1: (0.0, 2 * T)}[slope]
        return oracle.assign_threshold(np.ascontiguousarray(X, dtype=np.float32), slope, x_max, y_max)


@pytest.fixture
def restated_device(monkeypatch):
    """the host-array calls answered by the restatement"""
    from oracle import oracle
    monkeypatch.setattr(network, "query_links",
                        lambda i, j, lab, n_qry, max_links=8, device=0: links_restated(i, j, lab, n_qry, max_links))
    monkeypatch.setattr(network, "cluster_extend",
                        lambda i, j, lab, n_qry, device=0: extend_restated(i, j, lab, n_qry))
    monkeypatch.setattr(poppunk_refine, "generateTuples_array",
                        lambda a, w, self=True, num_ref=0, int_offset=0:
                        oracle.generate_tuples(np.asarray(a).astype(np.int32), w, self, num_ref, int_offset))
    monkeypatch.setattr(assign, "component_labels", labels_restated)
    monkeypatch.setattr(assign, "nearest_reference", knn1_restated)


def run_golden_case(case, z, tmp_path, capsys, model, to_device=None, labels=None):
    """assign_query_clusters on one golden case -> (result dict or None, stderr, exit code, error, query-query calls).
    to_device: None keeps numpy arrays, else a function that puts the matrix where the test wants it."""
    qNames = case["qNames"]
    qr, qq = z[case["name"] + "_qr"], z[case["name"] + "_qq"]
    index = {q: k for k, q in enumerate(qNames)}
    calls = []

    def queryDatabase(rNames, qNames, dbPrefix, queryPrefix, klist, self, number_plot_fits, threads):
        assert self and rNames == qNames
        calls.append(list(rNames))
        v, n = [index[x] for x in rNames], len(index)
        rows = [min(a, b) * n - min(a, b) * (min(a, b) + 1) // 2 + (max(a, b) - min(a, b) - 1)
                for x, a in enumerate(v) for b in v[x + 1:]]
        out = qq[np.array(rows, dtype=np.int64)].reshape(-1, 2)
        return to_device(out) if to_device else out

    opt = case["options"]
    output = str(tmp_path / "out")
    os.makedirs(output, exist_ok=True)
    old = str(tmp_path / "old_clusters.csv")
    open(old, "w").write(DOC["old_csv_large"] if opt.get("old_csv") == "large" else DOC["old_csv"])
    ref_edges = np.array(DOC["ref_edges"], dtype=np.int64).reshape(-1, 2)
    refnet = assign.ReferenceNetwork((to_device(ref_edges) if to_device else ref_edges, N_REF), DOC["rNames"], old,
                                     labels=labels)
    capsys.readouterr()
    res = code = error = None
    try:
        res = assign.assign_query_clusters({'queryDatabase': queryDatabase}, refnet, qNames,
                                           to_device(qr) if to_device else qr, model, output, kmers=[13, 17],
                                           qc_dict=opt.get("qc_dict"), serial=case["mode"] != "joint",
                                           stable=opt.get("stable"), update_db=opt.get("update_db", False),
                                           write_references=opt.get("write_references", False), return_network=True)
    except SystemExit as e:
        code = e.code
    except (ValueError, RuntimeError, KeyError) as e:
        error = [type(e).__name__, str(e)]
    return res, capsys.readouterr().err, code, error, calls, output


def check_golden_case(case, got, tmp_path):
    res, err, code, error, calls, output = got
    want = case["expected"]
    assert err == want["stderr"]
    assert code == want["exit"] and error == want["error"]
    assert calls == case["qq_calls"]
    if want["clustering"] is None:
        assert res is None
        return
    assert res["qNames"] == want["qNames_after"]
    clustering = res["isolateClustering"]["combined"] if case["mode"] == "joint" else res["isolateClustering"]
    assert clustering == want["clustering"]
    rows = [line.split(",") for line in open(os.path.join(output, "out_clusters.csv")).read().splitlines()[1:]]
    if case["mode"] == "joint":
        assert sorted(res["merged_queries"]) == want["merged"]
        assert (None if res["qqDistMat"] is None else list(res["qqDistMat"].shape)) == want["qq_shape"]
        edges = res["genomeNetwork"][0]
        edges = edges.cpu().numpy() if hasattr(edges, "is_cuda") else edges
        assert edges.tolist() == want["network_edges"]
        # inside a block the reference iterates a set: block order and membership are compared (network.printClusters)
        assert [r[1] for r in rows] == [r[1] for r in want["csv_rows"]]
        assert sorted(map(tuple, rows)) == sorted(map(tuple, want["csv_rows"]))
    else:
        assert rows == want["csv_rows"]


def test_fixture_covers_the_issue_list():
    e = {name: c["expected"] for name, c in CASES.items()}
    assert len(CASES) == 16 and all(len(c["qNames"]) in (1, 5, 6, 12) for c in CASES.values())
    assert "5_4" in e["joint_linked"]["clustering"].values()                  # a query merging two clusters
    assert "6_8_7" in e["joint_linked"]["clustering"].values()                # ... three
    assert e["joint_linked"]["qq_shape"] is None and "Found novel" not in e["joint_linked"]["stderr"]
    assert e["joint_unlinked"]["qq_shape"] == [66, 2] and "Found novel query clusters" in e["joint_unlinked"]["stderr"]
    c = e["joint_unlinked"]["clustering"]
    assert c["q07"] == c["q08"] and c["q07"] not in {c[r] for r in DOC["rNames"]}      # two novel queries, joined
    assert c["q09"] == c["q10"] == "2_1"                                      # query-query edges merge old clusters
    assert "2_1" not in e["joint_chain_not_asked"]["clustering"].values()     # ... only when they are computed
    assert "2_1" in e["joint_query_query"]["clustering"].values()             # queryQuery=True
    assert e["single_unlinked"]["qq_shape"] == [0, 2] and e["single_linked"]["qq_shape"] is None
    assert len(e["joint_linked_print_ref"]["csv_rows"]) == 52 and len(e["joint_linked"]["csv_rows"]) == 12
    assert "Running QC" not in e["qc_max_merge_1"]["stderr"]                  # upstream runs it for max_merge > 1 only
    assert e["qc_max_merge_2"]["qNames_after"] == [q for q in CASES["qc_max_merge_2"]["qNames"]
                                                   if q not in ("q09", "q11")]
    assert e["qc_all_fail"]["exit"] == 1
    assert 9 in e["serial_small_ids"]["clustering"].values()                  # a fresh id <= len(rNames) is not "novel"
    assert set(e["serial_large_ids"]["clustering"].values()) == {"novel"}     # ... and any id above it is
    # int('5_4') is 54 since Python 3.6 (the underscore separates digits): "novel", not the ValueError of older Pythons
    assert "have merged into 5_4" in e["serial_merged_name"]["stderr"] and e["serial_merged_name"]["error"] is None
    assert e["stable_core"]["clustering"] != e["stable_accessory"]["clustering"]
    assert "NA" in e["stable_core"]["clustering"].values()


@pytest.mark.parametrize("name", sorted(CASES))
def test_mirrors_match_the_reference_on_every_case(name, restated_device, tmp_path, capsys):
    case = CASES[name]
    check_golden_case(case, run_golden_case(case, arrays(), tmp_path, capsys, OracleModel()), tmp_path)


def test_labels_may_be_any_values_of_the_partition(restated_device, tmp_path, capsys):
    """the same partition under permuted label values gives the same result"""
    ref_edges = np.array(DOC["ref_edges"], dtype=np.int64)
    lab = labels_restated((ref_edges, N_REF))
    perm = np.random.default_rng(3).permutation(N_REF).astype(np.int32)
    case = CASES["joint_unlinked"]
    check_golden_case(case, run_golden_case(case, arrays(), tmp_path, capsys, OracleModel(), labels=perm[lab]),
                      tmp_path)


def test_add_query_to_network_on_its_own(restated_device, capsys):
    """the signature, the (G, qqDistMat) return and the RuntimeError of network.py:1362-1364"""
    case, z = CASES["joint_unlinked"], arrays()
    qr = z["joint_unlinked_qr"]
    model = OracleModel()
    G0 = (np.array(DOC["ref_edges"], dtype=np.int64), N_REF)
    with pytest.raises(RuntimeError, match="Must provide db querying info"):
        network.addQueryToNetwork({'queryDatabase': None}, DOC["rNames"], case["qNames"], G0, model.assign(qr), model,
                                  "db")
    qq = z["joint_unlinked_qq"]
    G, qqDistMat = network.addQueryToNetwork({'queryDatabase': lambda **kw: qq}, DOC["rNames"], case["qNames"], G0,
                                             model.assign(qr), model, "db", kmers=[13])
    assert G[1] == N_REF + 12 and len(G) == 2 and G[0].tolist() == case["expected"]["network_edges"]
    assert qqDistMat is qq
    assert capsys.readouterr().err == ("Found novel query clusters. Calculating distances between them.\n"
                                       "Calculating all query-query distances\n")


def test_weights_need_a_weighted_network(restated_device, capsys):
    case, z = CASES["joint_linked"], arrays()
    qr = z["joint_linked_qr"]
    model = OracleModel()
    ref_edges = np.array(DOC["ref_edges"], dtype=np.int64)
    with pytest.raises(SystemExit) as e:
        network.addQueryToNetwork({'queryDatabase': None}, DOC["rNames"], case["qNames"], (ref_edges, N_REF),
                                  model.assign(qr), model, "db", kmers=[13], weights=qr, distance_type='core')
    assert e.value.code == 1
    assert capsys.readouterr().err == ('Loaded network does not have edge weights; try a different network or turn off '
                                       'graph weights\n')
    old_w = np.full(ref_edges.shape[0], 0.5, dtype=np.float32)
    G, _ = network.addQueryToNetwork({'queryDatabase': None}, DOC["rNames"], case["qNames"],
                                     (ref_edges, N_REF, old_w), model.assign(qr), model, "db", kmers=[13], weights=qr,
                                     distance_type='core')
    m_new = G[0].shape[0] - ref_edges.shape[0]
    a = model.assign(qr)
    assert np.array_equal(G[2][:m_new], qr[a == -1, 0]) and np.array_equal(G[2][m_new:], old_w)
    G, _ = network.addQueryToNetwork({'queryDatabase': None}, DOC["rNames"], case["qNames"],
                                     (ref_edges, N_REF, old_w), a, model, "db", kmers=[13], weights=qr)
    assert np.array_equal(G[2][:m_new], np.linalg.norm(qr[a == -1], axis=1))


def test_qc_query_assignments(restated_device, tmp_path):
    case, z = CASES["qc_max_merge_2"], arrays()
    a = OracleModel().assign(z["qc_max_merge_2_qr"])
    old = str(tmp_path / "old.csv")
    open(old, "w").write(DOC["old_csv"])
    for max_clusters, failing in ((1, ["q08", "q09", "q11"]), (2, ["q09", "q11"]), (3, [])):
        retained, failed = qc.qcQueryAssignments(DOC["rNames"], case["qNames"], a, max_clusters, old)
        assert sorted(failed) == failing and retained == [q for q in case["qNames"] if q not in failing]
        assert all(v == ["Failed graph QC (too many links)"] for v in failed.values())
    open(old, "w").write("\n".join(DOC["old_csv"].split("\n")[:-3]) + "\n")         # two references fewer
    with pytest.raises(KeyError):
        qc.qcQueryAssignments(DOC["rNames"], case["qNames"], a, 2, old)


def test_serial_needs_every_reference_in_the_old_file(restated_device, tmp_path, capsys):
    case, z = CASES["serial_small_ids"], arrays()
    short = "\n".join(DOC["old_csv"].split("\n")[:-2]) + "\n"
    old = str(tmp_path / "old.csv")
    open(old, "w").write(short)
    refnet = assign.ReferenceNetwork((np.array(DOC["ref_edges"], dtype=np.int64), N_REF), DOC["rNames"], old)
    os.makedirs(str(tmp_path / "out"))
    with pytest.raises(NotImplementedError, match=DOC["rNames"][-1]):
        assign.assign_query_clusters({}, refnet, case["qNames"], z["serial_small_ids_qr"], OracleModel(),
                                     str(tmp_path / "out"), serial=True)


def test_reference_network_checks_the_vertex_count(restated_device, capsys):
    with pytest.raises(SystemExit):
        assign.ReferenceNetwork((np.zeros((0, 2), dtype=np.int64), N_REF + 1), DOC["rNames"], "unused")
    assert "vertices in the network but 40 reference names supplied" in capsys.readouterr().err


def test_restatement_on_a_worked_example():
    # references 0..5 in components {0, 3}, {1}, {2, 4, 5} (labels 3, 1, 0); queries 6, 7, 8
    lab = np.array([3, 1, 0, 3, 0, 0], dtype=np.int32)
    i = np.array([6, 0, 2, 7, 8, 1], dtype=np.int64)
    j = np.array([3, 6, 6, 8, 4, 0], dtype=np.int64)          # (1, 0) is reference-reference, (7, 8) query-query
    degree, n_links, links = links_restated(i, j, lab, 3, 2)
    assert degree.tolist() == [3, 0, 1] and n_links.tolist() == [2, 0, 1]
    assert links.tolist() == [[0, 3], [-1, -1], [0, -1]]
    assert links_restated(i, j, lab, 3, 1)[2].tolist() == [[0], [-1], [0]]
    numbers, count = extend_restated(i, j, lab, 3)
    assert count == 1 and numbers.tolist() == [1] * 9          # (1, 0) joins the last component too
    numbers, count = extend_restated(i[:5], j[:5], lab, 3)
    assert count == 2 and numbers.tolist() == [1, 2, 1, 1, 1, 1, 1, 1, 1]
    numbers, count = extend_restated(i[:0], j[:0], lab, 3)
    # sizes 2, 1, 3, 1, 1, 1 in lowest-vertex order: size descending, equal sizes by component index descending
    assert count == 6 and numbers.tolist() == [2, 6, 1, 2, 1, 1, 5, 4, 3]


def test_new_symbols_are_bound():
    for name in ("ppk_query_links_dev", "ppk_query_links", "ppk_cluster_extend_dev", "ppk_cluster_extend"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    src = open(os.path.join(os.path.dirname(HERE), "include", "ppk.h")).read()
    assert "#define PPK_ASSIGN_SET_CAP 128" in src


def test_argument_errors_need_no_device():
    with pytest.raises(RuntimeError, match="max_links must be 1 .. 64"):
        network.query_links([40], [0], np.zeros(40, dtype=np.int32), 1, max_links=0)
    with pytest.raises(RuntimeError, match="max_links must be 1 .. 64"):
        network.query_links([40], [0], np.zeros(40, dtype=np.int32), 1, max_links=65)
    lib = _lib.lib()                                  # (no arrays of that size: the check comes before any is read)
    with pytest.raises(RuntimeError, match=r"ppk_query_links: n_ref \+ n_qry must be < 2\^31"):
        _lib.check(lib.ppk_query_links(None, None, 0, None, 4, 2 ** 31 - 4, 8, 0, None, None, None), "x")
    with pytest.raises(RuntimeError, match=r"ppk_cluster_extend: n_ref \+ n_qry must be < 2\^31"):
        _lib.check(lib.ppk_cluster_extend(None, None, 0, None, 2 ** 31 - 4, 4, 0, None, None), "x")
    with pytest.raises(RuntimeError, match="ppk_query_links: NULL array"):
        _lib.check(lib.ppk_query_links(None, None, 3, None, 4, 2, 8, 0, None, None, None), "x")
    with pytest.raises(RuntimeError, match="ppk_cluster_extend: NULL array"):
        _lib.check(lib.ppk_cluster_extend(None, None, 3, None, 4, 2, 0, None, None), "x")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_the_twins_fail_loudly_without_a_device():
    lab = np.zeros(4, dtype=np.int32)
    with pytest.raises(RuntimeError):
        network.query_links([4], [0], lab, 1)
    with pytest.raises(RuntimeError):
        network.cluster_extend([4], [0], lab, 1)
