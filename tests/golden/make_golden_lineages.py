#!/usr/bin/env python3
"""Generates tests/golden/lineages.npz and tests/golden/lineages_csv.json: what the reference's own Python writes for
`poppunk_lineages --create-db` on a known matrix.

Run in the BUILD container only (needs the reference checkout, networkx, pandas and scipy); what it writes is data
(a distance matrix of this generator's making, name lists, CSV texts, COO arrays, pickled field values, stderr texts)
and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast`, as make_golden_clusters.py does, and run unmodified):
  PopPUNK/lineages.py   get_options, create_db, print_overall_clustering
  PopPUNK/models.py     ClusterFit, LineageFit (fit, assign, save, __save_sparse__, __reduce_rank__), reduce_rank,
                        rankFile
  PopPUNK/network.py    construct_network_from_edge_list, printClusters
  PopPUNK/plot.py       writeClusterCsv
  PopPUNK/utils.py      createOverallLineage, isolateNameToLabel, storePickle
under the real pandas / numpy / scipy of this image.  Stand-ins: pp_sketchlib.queryDatabase slices the known matrix
(rows of the strain's names, in the order given); pp_sketchlib.longToSquare and poppunk_refine.get_kNN_distances /
lowerRank are the oracle's restatements (oracle.long_to_square, knn, lower_rank: the C++ cannot be built here);
make_golden_clusters.py's networkx stand-in for graph-tool, here accepting an edge in both directions, which the
lineage networks hold; save_network does nothing; readDBParams returns fixed values.

The case: n = 300, network_sweep.npz's sweep1d matrix with both columns rounded to multiples of 2^-12 (rows then hold
duplicated distances and zeros), clusters.npz's multi_numbers[2] as the strains (sizes 35 .. 1), --min-count 11 (one
strain has exactly 11 members, the next 7), the clusters CSV in a shuffled row order.  Run once with default flags and
once with --reciprocal-only --count-unique-distances --use-accessory --ranks 1,2,5 --max-search-depth 8.

printClusters fills its dict by iterating Python sets of names, so the ROW ORDER of the combined CSV inside one
lineage of the first rank depends on the interpreter's string hash seed; the texts are recorded as written, and the
tests compare them block by block (tests/lineage_golden.py)."""
import ast
import contextlib
import io
import json
import os
import pickle
import shutil
import sys
import tempfile
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_clusters as mgc         # noqa: E402
import make_golden_network as mgn          # noqa: E402
from oracle import oracle                  # noqa: E402

REF = mgn.REF
N = 300
MIN_COUNT = 11
RUNS = {"default": [],
        "flags": ["--reciprocal-only", "--count-unique-distances", "--use-accessory", "--ranks", "1,2,5",
                  "--max-search-depth", "8"]}


def extract_classes(path, names, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    missing = [n for n in names if n not in namespace]
    if missing:
        raise RuntimeError("not found in %s: %s" % (path, missing))


class _Gt(mgc._Gt):
    class Graph(mgc._Gt.Graph):
        def add_edge_list(self, edge_list):
            for a, b in edge_list:
                self.g.add_edge(int(a), int(b))


def the_case():
    dist = np.load(os.path.join(HERE, "network_sweep.npz"))["sweep1d_dist"].astype(np.float32)
    dist = (np.round(dist.astype(np.float64) * 4096) / 4096).astype(np.float32)
    numbers = np.load(os.path.join(HERE, "clusters.npz"))["multi_numbers"][2]
    names = ["assemblies/s%03d.fa" % k for k in range(N)]
    order = np.random.default_rng(12).permutation(N)
    return dist, numbers, names, order


def reference_namespace(dist, names):
    import argparse

    import pandas as pd
    import scipy
    import scipy.sparse
    from pandas.errors import DataError
    index = {name: k for k, name in enumerate(names)}

    class _Sketchlib:
        @staticmethod
        def queryDatabase(ref_db_name, query_db_name, rList, qList, klist, random_correct, jaccard, num_threads,
                          use_gpu, device_id):
            assert rList == qList
            mem = np.asarray([index[name] for name in rList], dtype=np.int64)
            a, b = np.triu_indices(len(mem), 1)
            lo, hi = np.minimum(mem[a], mem[b]), np.maximum(mem[a], mem[b])
            return np.ascontiguousarray(dist[lo * (2 * N - lo - 1) // 2 + (hi - lo - 1)])

        @staticmethod
        def longToSquare(distVec, num_threads=1):
            return oracle.long_to_square(distVec)

    class _Refine:
        @staticmethod
        def get_kNN_distances(distMat, kNN, dist_col, num_threads):
            return oracle.knn(distMat, kNN)

        @staticmethod
        def lowerRank(mat, n_samples, kNN, reciprocal_only, count_unique_distances, resolution, num_threads):
            return oracle.lower_rank(mat[0], mat[1], mat[2], n_samples, kNN, reciprocal_only, count_unique_distances,
                                     resolution)

    ns = mgc.reference_namespace()
    ns.update({"argparse": argparse, "pd": pd, "scipy": scipy, "pickle": pickle, "shutil": shutil, "os": os, "sys": sys,
               "defaultdict": defaultdict, "DataError": DataError, "gt": _Gt, "pp_sketchlib": _Sketchlib,
               "poppunk_refine": _Refine, "epsilon": 1e-10, "SEARCH_DEPTH_FACTOR": 10,
               "DEFAULT_LINEAGE_RESOLUTION": 1e-10,
               "save_network": lambda *a, **kw: None,
               "readDBParams": lambda db: (np.asarray([13, 17, 21, 25, 29]), 156, False)})
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "utils.py"),
                          ["createOverallLineage", "isolateNameToLabel", "storePickle"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "plot.py"), ["writeClusterCsv"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "models.py"), ["reduce_rank", "rankFile"], ns)
    extract_classes(os.path.join(REF, "PopPUNK", "models.py"), ["ClusterFit"], ns)
    extract_classes(os.path.join(REF, "PopPUNK", "models.py"), ["LineageFit"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "lineages.py"),
                          ["get_options", "create_db", "print_overall_clustering"], ns)
    return ns


def coo_of(path):
    import scipy.sparse
    m = scipy.sparse.load_npz(path).tocoo()
    return m.row.astype(np.int64), m.col.astype(np.int64), m.data.astype(np.float32)


def main():
    dist, numbers, names, order = the_case()
    ns = reference_namespace(dist, names)
    arrays = {"dist": dist, "strain_numbers": numbers.astype(np.int32), "csv_order": order.astype(np.int64)}
    texts = {"names": names, "min_count": MIN_COUNT, "runs": {}}
    csv_text = "Taxon,Cluster\n" + "".join("%s,%d\n" % (names[k], numbers[k]) for k in order)
    texts["clusters_csv"] = csv_text
    cwd = os.getcwd()
    for run, flags in RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                os.makedirs("db")
                with open(os.path.join("db", "db_clusters.csv"), "w") as f:
                    f.write(csv_text)
                argv = ["poppunk_lineages", "--create-db", "db", "--db-scheme", "scheme.pkl", "--output", "out",
                        "--min-count", str(MIN_COUNT)] + flags
                err = io.StringIO()
                old_argv = sys.argv
                sys.argv = argv
                try:
                    with contextlib.redirect_stderr(err):
                        ns["create_db"](ns["get_options"]())
                finally:
                    sys.argv = old_argv
                rec = {"argv": argv[1:], "stderr": err.getvalue(), "out_csv": open("out.csv").read(), "strains": {}}
                with open("scheme.pkl", "rb") as f:
                    scheme = pickle.load(f)
                rec["scheme"] = [v.tolist() if isinstance(v, np.ndarray) else v for v in scheme]
                for strain, db_name in scheme[18].items():
                    stem = os.path.join(db_name, db_name)
                    with open(stem + "_fit.pkl", "rb") as f:
                        fit = pickle.load(f)
                    with open(stem + ".dists.pkl", "rb") as f:
                        names_pkl = pickle.load(f)
                    rec["strains"][strain] = {"db": db_name, "lineages_csv": open(stem + "_lineages.csv").read(),
                                              "fit_pkl": fit, "names_pkl": names_pkl,
                                              "h5_link": os.readlink(stem + ".h5"),
                                              "files": sorted(os.listdir(db_name))}
                    for what, path in [("nn", stem + "_sparse_dists.npz")] + [
                            ("rank%d" % r, stem + ns["rankFile"](r)) for r in fit[0][0]]:
                        r_, c_, d_ = coo_of(path)
                        key = "%s_%s_%s_" % (run, strain, what)
                        arrays[key + "row"], arrays[key + "col"], arrays[key + "data"] = r_, c_, d_
                texts["runs"][run] = rec
            finally:
                os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, "lineages.npz"), **arrays)
    with open(os.path.join(HERE, "lineages_csv.json"), "w") as f:
        json.dump(texts, f, indent=1)
    print({run: (len(rec["strains"]), len(rec["out_csv"].splitlines())) for run, rec in texts["runs"].items()})


if __name__ == "__main__":
    main()
