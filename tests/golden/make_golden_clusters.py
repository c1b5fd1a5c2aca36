#!/usr/bin/env python3
"""Generates tests/golden/clusters.npz and tests/golden/clusters_csv.json: cluster numbers, names and the iterate
family as the reference computes them.

Run in the BUILD container only (needs the reference checkout, networkx, pandas and scipy); what it writes is data
(edge lists, number arrays, CSV texts of this generator's own making, expected dicts and lists, stderr texts, file
indices, label matrices, means) and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast`, as make_golden_network.py does, and run unmodified):
  PopPUNK/network.py          printClusters, printExternalClusters, construct_network_from_df,
                              construct_network_from_edge_list, networkSummary
  PopPUNK/utils.py            readIsolateTypeFromCsv, transformLine, decisionBoundary
  PopPUNK/refine.py           multi_refine, growNetwork, check_search_range
  scripts/poppunk_iterate.py  read_next_cluster_file, is_nested, and the statements of its main block that build the
                              family (:156-182) and Avg_Pi (:195-215)
under the real pandas / numpy / scipy of this image and make_golden_network.py's networkx stand-in for graph-tool,
whose label_components is extended HERE to return `.a`, every vertex's component numbered in the order of the
components' lowest vertices -- that graph-tool numbers them so is UNVERIFIED.  The oracle's threshold_iterate_1d stands
in for poppunk_refine.thresholdIterate1D, and a stand-in queryDatabase slices the known distance matrix.

clusters_csv.json: `naming`, a list of cases {name, n, edges, names, old_csv, ext_csv, printRef, numbers, clustering,
merged, stderr, csv_rows, ext_csv_out, error}; `read_csv`, readIsolateTypeFromCsv's results on small CSV texts.
clusters.npz:
  multi_*    multi_refine on network_sweep.npz's n = 300 matrix: mean0, mean1, s_max, n_points, file_idx, numbers
             int32 [n_files, n]
  holes_*    growNetwork(write_clusters=...) on network_sweep.npz's `holes` triples: file_idx, numbers, edge_counts
  iter_*     the iterate family on multi_refine's files: ids, sizes, members (a [n_family, n] 0/1 matrix), sorted
             (the ids, size descending), avg_pi (the reference's float32 means, as float64), allowance = twice the
             largest |float32 np.mean - float64 mean| over the family (the reference side's own summation error)
"""
import ast
import contextlib
import io
import json
import operator
import os
import sys
import tempfile
from collections import Counter, defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_network as mgn          # noqa: E402

REF = mgn.REF


class _Assignments:
    def __init__(self, a):
        self.a = a


class _Gt(mgn._FakeGt):
    @staticmethod
    def label_components(g):
        import networkx as nx
        comps = sorted(nx.connected_components(g.g), key=min)
        a = np.zeros(g.g.number_of_nodes(), dtype=np.int64)
        for k, c in enumerate(comps):
            a[list(c)] = k
        return _Assignments(a), np.array([len(c) for c in comps], dtype=np.int64)


def reference_namespace(thresholder=None):
    import pandas as pd
    from math import sqrt
    from scipy.stats import rankdata

    class _Refine:
        @staticmethod
        def thresholdIterate1D(distMat, s_range, slope, x0, y0, x1, y1, num_processes=1):
            i, j, o = thresholder(distMat, np.asarray(s_range, dtype=np.float64), slope, x0, y0, x1, y1)
            return i.tolist(), j.tolist(), o.tolist()

    ns = {"np": np, "pd": pd, "gt": _Gt, "tqdm": mgn._Tqdm, "os": os, "sys": sys, "sqrt": sqrt,
          "rankdata": rankdata, "Counter": Counter, "operator": operator, "defaultdict": defaultdict,
          "betweenness_sample_default": 100, "poppunk_refine": _Refine}
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "utils.py"),
                          ["readIsolateTypeFromCsv", "transformLine", "decisionBoundary"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "network.py"),
                          ["construct_network_from_df", "construct_network_from_edge_list", "networkSummary",
                           "printClusters", "printExternalClusters"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "refine.py"),
                          ["multi_refine", "growNetwork", "check_search_range"], ns)
    return ns


def graph_of(ns, n, edges):
    g = _Gt.Graph(directed=False)
    g.add_vertex(n)
    g.add_edge_list([tuple(e) for e in edges])
    return g


def numbers_of(n, edges):
    """the reference's ranking on the stand-in's components (what printClusters computes before it names anything)"""
    from scipy.stats import rankdata
    g = graph_of(None, n, edges)
    assign, freq = _Gt.label_components(g)
    ranks = len(freq) - rankdata(freq, method='ordinal').astype(int)
    return (ranks[assign.a] + 1).astype(int).tolist()


def read_rows(path):
    with open(path) as f:
        lines = f.read().splitlines()
    return [line.split(",") for line in lines[1:]]


def naming_case(ns, name, n, edges, old_csv=None, ext_csv=None, printRef=True):
    names = ["s%02d" % k for k in range(n)]
    case = {"name": name, "n": n, "edges": [list(map(int, e)) for e in edges], "names": names, "old_csv": old_csv,
            "ext_csv": ext_csv, "printRef": printRef, "numbers": numbers_of(n, edges), "clustering": None,
            "merged": None, "stderr": "", "csv_rows": None, "ext_csv_out": None, "error": None}
    with tempfile.TemporaryDirectory() as tmp:
        old_path = ext_path = None
        if old_csv is not None:
            old_path = os.path.join(tmp, "old.csv")
            open(old_path, "w").write(old_csv)
        if ext_csv is not None:
            ext_path = os.path.join(tmp, "ext.csv")
            open(ext_path, "w").write(ext_csv)
        err = io.StringIO()
        try:
            with contextlib.redirect_stderr(err):
                clustering, merged = ns["printClusters"](graph_of(ns, n, edges), names,
                                                         outPrefix=os.path.join(tmp, "out"), oldClusterFile=old_path,
                                                         externalClusterCSV=ext_path, printRef=printRef,
                                                         write_unwords=False)
        except RuntimeError as e:
            case["error"] = str(e)
            return case
        case["clustering"] = {k: (int(v) if not isinstance(v, str) else v) for k, v in clustering.items()}
        case["merged"] = sorted(merged)
        case["stderr"] = err.getvalue()
        case["csv_rows"] = read_rows(os.path.join(tmp, "out_clusters.csv"))
        ext_out = os.path.join(tmp, "out_external_clusters.csv")
        if os.path.exists(ext_out):
            case["ext_csv_out"] = [line.split(",") for line in open(ext_out).read().splitlines()]
    return case


def old_csv_of(assign):
    return "Taxon,Cluster\n" + "".join("s%02d,%s\n" % (k, c) for k, c in assign)


def naming_cases(ns):
    # 12 samples: components {0,1,2,3}, {4,5,6}, {7,8}, {9}, {10}, {11} unless a case says otherwise
    base = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (7, 8)]
    out = [naming_case(ns, "no_old_file", 12, base)]
    # old file: samples 0-8 known; 9-11 are new
    exact = [(0, "1"), (1, "1"), (2, "1"), (3, "1"), (4, "2"), (5, "2"), (6, "2"), (7, "3"), (8, "3")]
    out.append(naming_case(ns, "exact_match", 12, base, old_csv_of(exact)))
    # two old clusters joined by the new sample 9
    out.append(naming_case(ns, "merge_two", 12, base + [(3, 9), (9, 4)], old_csv_of(exact)))
    # three old clusters joined, met in the old file's order (2, 3, 1)
    reordered = [(4, "2"), (5, "2"), (6, "2"), (7, "3"), (8, "3"), (0, "1"), (1, "1"), (2, "1"), (3, "1")]
    out.append(naming_case(ns, "merge_three", 12, base + [(3, 9), (9, 4), (6, 10), (10, 7)], old_csv_of(reordered)))
    # old cluster 1 = {0,1,2,3} now in two components
    out.append(naming_case(ns, "split", 12, [(0, 1), (2, 3), (4, 5), (5, 6), (7, 8)], old_csv_of(exact)))
    # old names include a merged id 4_6: a cluster of only new names must skip 4, 6 and take 7
    merged_old = [(0, "1"), (1, "1"), (2, "1"), (3, "1"), (4, "4_6"), (5, "4_6"), (6, "4_6"), (7, "3"), (8, "3")]
    out.append(naming_case(ns, "new_names_with_merged_ids", 12, base + [(9, 10)], old_csv_of(merged_old)))
    out.append(naming_case(ns, "print_ref_false", 12, base + [(3, 9)], old_csv_of(exact), printRef=False))
    out.append(naming_case(ns, "no_old_file_no_ref", 12, base, printRef=False))
    ext = "sample,MLST,Serotype,ignored\n" + "".join(
        "s%02d,%s,%s,x\n" % (k, m, s) for k, m, s in [(0, "ST1", "19A"), (1, "ST1", "19A"), (2, "ST2", "19A"),
                                                    (4, "ST5", "3"), (7, "ST9", "6B"), (9, "ST7", "14")])
    out.append(naming_case(ns, "external", 12, base, old_csv_of(exact), ext_csv=ext))
    return out


def read_csv_cases(ns):
    texts = {
        "clusters": "Taxon,Cluster,Cluster_b__autocolour,Other\na,1,x,p\nb,1,y,q\nc,2,y,r\n",
        "lineages": "id,Rank_1_Lineage,Rank_2_Lineage,overall_Lineage,note\na,1,1,1-1,p\nb,1,2,1-2,q\n",
        "external_one": "sample,Type\na,t1\nb,t2\nc,t1\n",
        "external_many": "sample,A,B,last\na,a1,b1,z\nb,a1,b2,z\nc,a2,b2,z\n",
    }
    mode_of = {"clusters": "clusters", "lineages": "lineages", "external_one": "external", "external_many": "external"}
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in texts.items():
            path = os.path.join(tmp, name + ".csv")
            open(path, "w").write(text)
            sets = ns["readIsolateTypeFromCsv"](path, mode=mode_of[name], return_dict=False)
            dicts = ns["readIsolateTypeFromCsv"](path, mode=mode_of[name], return_dict=True)
            out.append({"name": name, "mode": mode_of[name], "text": text,
                        "sets": [[col, [[k, sorted(map(str, v))] for k, v in d.items()]] for col, d in sets.items()],
                        "dicts": [[col, [[k, v] for k, v in d.items()]] for col, d in dicts.items()]})
    return out


def files_of(prefix, names):
    """(file indices, numbers [n_files, n]) of the _boundary<k>_clusters.csv files under prefix"""
    base = os.path.join(prefix, os.path.basename(prefix))
    index = {name: v for v, name in enumerate(names)}
    idx, rows = [], []
    for k in range(2000):
        path = "%s_boundary%d_clusters.csv" % (base, k)
        if not os.path.exists(path):
            continue
        row = np.zeros(len(names), dtype=np.int32)
        for name, c in read_rows(path):
            row[index[name]] = int(c)
        assert (row > 0).all()
        idx.append(k)
        rows.append(row)
    return np.array(idx, dtype=np.int64), np.stack(rows)


def iterate_family(db_dir, names, dist):
    """the script's family and Avg_Pi statements, run on the files under db_dir"""
    path = os.path.join(REF, "scripts", "poppunk_iterate.py")
    tree = ast.parse(open(path).read())
    index = {name: v for v, name in enumerate(names)}
    n = len(names)

    class _Sketchlib:
        @staticmethod
        def queryDatabase(ref, query, rNames, qNames, kmers, random_correct, jaccard, cpus, use_gpu, deviceid):
            assert rNames == qNames
            v = [index[x] for x in rNames]
            rows = []
            for a in range(len(v)):
                for b in range(a + 1, len(v)):
                    lo, hi = min(v[a], v[b]), max(v[a], v[b])
                    rows.append(lo * n - lo * (lo + 1) // 2 + (hi - lo - 1))
            return dist[np.array(rows, dtype=np.int64)]

    class _Args:
        db = db_dir
        h5 = "unused"
        cpus = 1

    ns = {"np": np, "os": os, "defaultdict": defaultdict, "pp_sketchlib": _Sketchlib, "args": _Args,
          "stderr_redirected": contextlib.nullcontext, "kmers": None, "random_correct": True, "jaccard": False,
          "use_gpu": False, "deviceid": 0}
    mgn.extract_functions(path, ["read_next_cluster_file", "is_nested"], ns)
    main = [node for node in tree.body if isinstance(node, ast.If)][-1]
    src = open(path).read()
    texts = [ast.get_source_segment(src, st) for st in main.body]
    first = next(k for k, t in enumerate(texts) if t.startswith("db_name ="))
    last = next(k for k, t in enumerate(texts) if t.startswith("sorted_clusters ="))
    pi0 = next(k for k, t in enumerate(texts) if t.startswith("pi_values ="))
    pi1 = next(k for k, t in enumerate(texts) if t.startswith("with stderr_redirected()"))
    body = main.body[first:last + 1] + main.body[pi0:pi1 + 1]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    family, order, pi = ns["iterated_clusters"], ns["sorted_clusters"], ns["pi_values"]
    ids = np.array(list(family.keys()), dtype=np.int64)
    members = np.zeros((ids.size, n), dtype=np.uint8)
    err = 0.0
    for r, c in enumerate(ids.tolist()):
        members[r, [index[x] for x in family[c]]] = 1
        d = _Sketchlib.queryDatabase(None, None, list(family[c]), list(family[c]), None, True, False, 1, False, 0)[:, 0]
        err = max(err, abs(float(np.mean(d)) - float(np.mean(d.astype(np.float64)))))
    return {"ids": ids, "members": members, "sizes": members.sum(axis=1).astype(np.int64),
            "sorted": np.array(order, dtype=np.int64),
            "avg_pi": np.array([float(pi[c]) for c in ids.tolist()], dtype=np.float64),
            "allowance": np.float64(2.0 * err)}


def main():
    from oracle import oracle
    ns = reference_namespace(oracle.threshold_iterate_1d)
    doc = {"naming": naming_cases(ns), "read_csv": read_csv_cases(ns)}
    with open(os.path.join(HERE, "clusters_csv.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")

    out = {}
    z = np.load(os.path.join(HERE, "network_sweep.npz"))
    dist = z["sweep1d_dist"]
    n = int(z["sweep1d_n"])
    names = ["s%d" % k for k in range(n)]
    x1, y1 = float(z["sweep1d_line"][2]), float(z["sweep1d_line"][3])
    mean0, mean1 = np.array([0.15 * x1, 0.2 * y1]), np.array([x1, y1])
    s_max = 0.55 * float(np.hypot(*(mean1 - mean0)))
    n_points = 12
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "multi")
        os.makedirs(prefix)
        with contextlib.redirect_stderr(io.StringIO()):
            ns["multi_refine"](dist, names, mean0, mean1, np.array([1.0, 1.0]), s_max, n_points, prefix)
        idx, numbers = files_of(prefix, names)
        out.update(multi_mean0=mean0, multi_mean1=mean1, multi_s_max=np.float64(s_max),
                   multi_n_points=np.int64(n_points), multi_file_idx=idx, multi_numbers=numbers)
        fam = iterate_family(prefix, names, dist)
        out.update({"iter_" + k: v for k, v in fam.items()})

    i, j, o, hn = z["holes_i"], z["holes_j"], z["holes_idx"], int(z["holes_n"])
    hnames = ["s%d" % k for k in range(hn)]
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "holes")
        os.makedirs(prefix)
        n_off = int(o.max()) + 1
        ns["growNetwork"](hnames, i.tolist(), j.tolist(), o.tolist(), list(range(n_off)), 0, write_clusters=prefix)
        idx, numbers = files_of(prefix, hnames)
        out.update(holes_file_idx=idx, holes_numbers=numbers,
                   holes_edge_counts=np.bincount(o, minlength=n_off).astype(np.int64))

    np.savez_compressed(os.path.join(HERE, "clusters.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", v))
    print("naming cases:", [c["name"] for c in doc["naming"]])
    print("family:", fam["ids"].size, "clusters; allowance", float(fam["allowance"]))


if __name__ == "__main__":
    main()
