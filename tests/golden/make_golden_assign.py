#!/usr/bin/env python3
"""Generates tests/golden/assign.json and tests/golden/assign.npz: poppunk_assign's last step as the reference
computes it, on loaded pieces.

Run in the BUILD container only (needs the reference checkout, networkx, pandas and scipy); what it writes is data
(names, edge lists, CSV texts of this generator's own making, distance matrices of its own making, expected dicts,
lists, stderr texts, CSV rows and error texts) and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast`, as make_golden_clusters.py does, and run unmodified):
  PopPUNK/network.py   addQueryToNetwork, construct_network_from_assignments, construct_network_from_edge_list,
                       process_previous_network, network_to_edges, process_weights, printClusters
  PopPUNK/qc.py        qcQueryAssignments, prune_query_distance_matrix
  PopPUNK/utils.py     readIsolateTypeFromCsv
  PopPUNK/assign.py    the statements of assign_query_hdf5 at :592-733 (everything after the vertex-count check of the
                       non-lineage branch, up to and including the CSV of the serial / stable modes)
under the real pandas / numpy / scipy of this image.  Stand-ins:
  graph-tool           make_golden_clusters.py's networkx stand-in, extended HERE with what these functions need:
                       get_total_degrees, copy, edge_endpoint_property, vertex_index, edge_properties (always empty: no
                       case carries weights) and an edge list kept in insertion order
  poppunk_refine       generateTuples = the oracle's; get_kNN_distances = a numpy restatement of src/extend.cpp:248-289
                       (ascending by distance, ties by index, column i of row i skipped -- in a rectangle too)
  queryDatabase        a slice of the case's known query-query matrix
  the model            assign = the oracle's threshold (assign_threshold) with within_label = -1, type 'refine'
  addRandom, tqdm, gen_unword   no-ops (gen_unword yields names that only go to a file nobody reads)
`from .utils import readIsolateTypeFromCsv` inside the extracted statements is served by a stand-in package whose
utils module holds the extracted function.

serial_merged_name records what Python makes of int('5_4'): 54 since Python 3.6 (the underscore separates digits), so
the merged name becomes "novel" and no ValueError is raised.

One line of stderr is canonicalised: upstream joins a frozenset of failed sample names, whose order follows the
hash seed; the recorded line lists them in query order.

Every case: 40 references in 8 clusters (the reference network is the threshold's own self edges, the old cluster file
printClusters' on it) and up to 12 queries placed in a 2-D latent space (core = Euclidean distance there, accessory =
2 core + a little) so that each does what its name says.  For the `stable` cases the generator asserts that every
query's minimum is unique.

assign.json: {"x_max", "y_max", "rNames", "ref_edges", "old_csv", "old_csv_large", "cases": [...]}; a case: {name, mode
(joint | serial | stable), qNames, options, expected: {clustering, merged, stderr, csv_rows, error, exit,
network_edges, qq_shape, qNames_after}}.  assign.npz: <case>_qr float32 [n_qry * 40, 2], <case>_qq float32 condensed.
"""
import ast
import contextlib
import io
import json
import operator
import os
import sys
import tempfile
import types
from collections import Counter, defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_clusters as mgc         # noqa: E402
import make_golden_network as mgn          # noqa: E402

REF = mgn.REF
T = 0.01                                   # the within-strain scale of the latent space
X_MAX, Y_MAX = 2 * T, 4 * T                # slope 2: c / X_MAX + a / Y_MAX <= 1  <=>  c <= T - e / 4 for a = 2 c + e
N_REF = 40


class _Graph(mgc._Gt.Graph):
    def __init__(self, directed=False):
        super().__init__(directed)
        self.elist = []
        self.edge_properties = {}
        self.vertex_index = "vertex_index"

    def add_edge_list(self, edge_list, eprops=None):
        edge_list = [tuple(int(v) for v in e) for e in edge_list]
        super().add_edge_list(edge_list)
        self.elist.extend(edge_list)

    def get_total_degrees(self, vs):
        return np.array([self.g.degree(v) for v in vs], dtype=np.int64)

    def copy(self):
        g = _Graph()
        g.add_vertex(self.g.number_of_nodes())
        g.add_edge_list(self.elist)
        return g


class _Gt(mgc._Gt):
    Graph = _Graph

    @staticmethod
    def edge_endpoint_property(g, prop, which):
        assert prop == g.vertex_index
        return [e[0 if which == "source" else 1] for e in g.elist]


def knn_restated(distMat, kNN, dist_col=0, num_threads=1):
    i_vec, j_vec, dists = [], [], []
    for i in range(distMat.shape[0]):
        row = distMat[i]
        order = [int(j) for j in np.argsort(row, kind="stable") if j != i][:kNN]
        i_vec += [i] * kNN
        j_vec += order
        dists += [float(row[j]) for j in order]
    return i_vec, j_vec, dists


class Model:
    type = 'refine'
    threshold = False
    within_label = -1

    def assign(self, X, slope=2):
        from oracle import oracle
        x_max, y_max = {2: (X_MAX, Y_MAX), 0: (T, 0.0), 1: (0.0, 2 * T)}[slope]
        return oracle.assign_threshold(np.ascontiguousarray(X, dtype=np.float32), slope, x_max, y_max)


def reference_namespace():
    import pandas as pd
    from scipy.stats import rankdata
    from oracle import oracle

    def generateTuples(assignments, within_label, self=True, num_ref=0, int_offset=0):
        return [tuple(e) for e in oracle.generate_tuples(np.asarray(assignments).astype(np.int32), within_label, self,
                                                         num_ref, int_offset).tolist()]

    refine_mod = types.ModuleType("poppunk_refine")
    refine_mod.generateTuples = generateTuples
    refine_mod.get_kNN_distances = knn_restated
    sys.modules["poppunk_refine"] = refine_mod           # (`import poppunk_refine` inside the stable branch)

    def gen_unword():
        k = 0
        while True:
            k += 1
            yield "unword%d" % k

    ns = {"np": np, "pd": pd, "gt": _Gt, "tqdm": lambda it, **kw: it, "os": os, "sys": sys, "rankdata": rankdata,
          "Counter": Counter, "operator": operator, "itemgetter": operator.itemgetter, "defaultdict": defaultdict,
          "betweenness_sample_default": 100, "poppunk_refine": refine_mod, "gen_unword": gen_unword,
          "addRandom": lambda *a, **kw: None, "accepted_weights_types": ["core", "euclidean", "accessory"],
          "__package__": "ppk_reference_standin", "__name__": "ppk_reference_standin.assign"}
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "utils.py"), ["readIsolateTypeFromCsv"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "network.py"),
                          ["addQueryToNetwork", "construct_network_from_assignments", "construct_network_from_edge_list",
                           "process_previous_network", "network_to_edges", "process_weights", "printClusters"], ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "qc.py"), ["qcQueryAssignments", "prune_query_distance_matrix"],
                          ns)
    pkg = types.ModuleType("ppk_reference_standin")
    pkg.__path__ = []
    utils_mod = types.ModuleType("ppk_reference_standin.utils")
    utils_mod.readIsolateTypeFromCsv = ns["readIsolateTypeFromCsv"]
    sys.modules["ppk_reference_standin"] = pkg
    sys.modules["ppk_reference_standin.utils"] = utils_mod
    return ns


def assign_body():
    """the statements of assign_query_hdf5 at :592-733, compiled as they stand"""
    path = os.path.join(REF, "PopPUNK", "assign.py")
    tree = ast.parse(open(path).read())
    fn = next(node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "assign_query_hdf5")
    loop = next(node for node in fn.body if isinstance(node, ast.For) and getattr(node.target, "id", "") == "fit_type")
    branch = next(node for node in loop.body if isinstance(node, ast.If)
                  and ast.unparse(node.test) == "model.type == 'lineage'")
    body = [st for st in branch.orelse if 592 <= st.lineno <= 733]
    assert body and ast.unparse(body[0].test).startswith("fit_type == 'core_refined'"), "the reference has moved"
    assert body[-1].end_lineno <= 733 and isinstance(body[-1], ast.If) and ast.unparse(body[-1].test) == "not serial"
    return compile(ast.Module(body=body, type_ignores=[]), path, "exec")


# ---- the data ------------------------------------------------------------------------------------------------------
SIZES = [8, 7, 6, 5, 5, 4, 3, 2]
S = 1.4 * T                                 # spacing of clusters a query can bridge
CENTRES = {"A": (0.0, 0.0), "B": (S, 0.0),                                   # a pair
           "D": (20 * T, 0.0), "E": (20 * T + S, 0.0),                      # a pair
           "F": (0.0, 20 * T), "G": (S, 20 * T), "H": (S / 2, 20 * T + S * np.sqrt(3) / 2),      # a triangle
           "C": (20 * T, 20 * T)}                                            # alone
ORDER = ["A", "B", "C", "D", "E", "F", "G", "H"]


def mid(*names):
    return tuple(np.mean([CENTRES[k] for k in names], axis=0))


def towards(a, b, frac_of_T):
    pa, pb = np.array(CENTRES[a]), np.array(CENTRES[b])
    return tuple(pa + (pb - pa) / np.linalg.norm(pb - pa) * frac_of_T * T)


def distances(pa, pb, rng, self_job):
    """float32 [rows, 2]: query-major rectangle (row q * n_ref + r) or the condensed triangle of pa"""
    if self_job:
        ii, jj = np.triu_indices(len(pa), 1)
        core = np.linalg.norm(pa[ii] - pa[jj], axis=1)
    else:
        core = np.linalg.norm(pb[:, None, :] - pa[None, :, :], axis=2).ravel()
    acc = 2 * core + rng.uniform(0.0, 0.2 * T, core.size)
    return np.stack([core, acc], axis=1).astype(np.float32)


def reference_set(rng):
    pos, member = [], []
    for name, size in zip(ORDER, SIZES):
        pos.append(np.array(CENTRES[name]) + rng.uniform(-0.02 * T, 0.02 * T, (size, 2)))
        member += [name] * size
    pos = np.concatenate(pos)
    perm = rng.permutation(N_REF)            # clusters are not contiguous in vertex order
    return pos[perm], [member[k] for k in perm]


def read_rows(path):
    return mgc.read_rows(path) if os.path.exists(path) else None


def canonical_stderr(text, qNames):
    lines = text.split("\n")
    for k, line in enumerate(lines):
        if k and lines[k - 1].endswith("samples failed:"):
            failed = set(line.split(","))
            lines[k] = ",".join(q for q in qNames if q in failed)
    return "\n".join(lines)


def run_case(ns, body, name, mode, rNames, ref_edges, old_csv, qpos, rpos, rng, options):
    from oracle import oracle                # noqa: F401
    qNames = ["q%02d" % k for k in range(len(qpos))]
    qpos = np.array(qpos, dtype=np.float64) + rng.uniform(-0.005 * T, 0.005 * T, (len(qpos), 2))
    qr = distances(rpos, qpos, rng, False)
    qq = distances(qpos, None, rng, True)
    index = {q: k for k, q in enumerate(qNames)}

    calls = []

    def queryDatabase(rNames, qNames, dbPrefix, queryPrefix, klist, self, number_plot_fits, threads):
        assert self and rNames == qNames
        calls.append(list(rNames))
        v = [index[x] for x in rNames]
        n = len(qpos)
        rows = [min(a, b) * n - min(a, b) * (min(a, b) + 1) // 2 + (max(a, b) - min(a, b) - 1)
                for x, a in enumerate(v) for b in v[x + 1:]]
        return qq[np.array(rows, dtype=np.int64)].reshape(-1, 2)

    if mode == "stable":
        col = 0 if options["stable"] == "core" else 1
        m = qr[:, col].reshape(len(qNames), N_REF).copy()
        for q in range(min(len(qNames), N_REF)):
            m[q, q] = np.inf
        srt = np.sort(m, axis=1)
        assert (srt[:, 0] < srt[:, 1]).all(), "a stable case has a tied minimum"

    expected = {"clustering": None, "merged": None, "stderr": "", "csv_rows": None, "error": None, "exit": None,
                "network_edges": None, "qq_shape": None, "qNames_after": None}
    with tempfile.TemporaryDirectory() as tmp:
        output = os.path.join(tmp, "out")
        os.makedirs(output)
        old_path = os.path.join(tmp, "old_clusters.csv")
        open(old_path, "w").write(old_csv)
        g = _Graph()
        g.add_vertex(N_REF)
        g.add_edge_list(ref_edges)
        run = dict(ns)
        run.update(fit_type='default', model=Model(), qrDistMat=qr, qc_dict=options.get("qc_dict", {'run_qc': False}),
                   rNames=list(rNames), qNames=list(qNames), old_cluster_file=old_path,
                   graph_weights=False, output=output, file_extension_string='', serial=mode != "joint",
                   stable=options.get("stable"), dbFuncs={'queryDatabase': queryDatabase}, genomeNetwork=g,
                   kmers=[13, 17], update_db=options.get("update_db", False), strand_preserved=False, threads=1,
                   gpu_graph=False, external_clustering=None, write_references=options.get("write_references", False))
        err = io.StringIO()
        try:
            with contextlib.redirect_stderr(err):
                exec(body, run)
        except SystemExit as e:
            expected["exit"] = e.code
        except (ValueError, RuntimeError, KeyError) as e:
            expected["error"] = [type(e).__name__, str(e)]
        expected["stderr"] = canonical_stderr(err.getvalue(), qNames)
        expected["qNames_after"] = run["qNames"]
        if expected["exit"] is None and expected["error"] is None:
            clustering = run["isolateClustering"]
            if mode == "joint":
                clustering = clustering["combined"]
                expected["merged"] = sorted(run["merged_queries"])
                expected["network_edges"] = [list(e) for e in run["genomeNetwork"].elist]
                qqd = run["qqDistMat"]
                expected["qq_shape"] = None if qqd is None else list(qqd.shape)
            expected["clustering"] = {k: (v if isinstance(v, str) else int(v)) for k, v in clustering.items()}
            expected["csv_rows"] = read_rows(os.path.join(output, "out_clusters.csv"))
    case = {"name": name, "mode": mode, "qNames": qNames, "options": options, "expected": expected,
            "qq_calls": calls}
    return case, qr, qq


def main():
    from oracle import oracle
    rng = np.random.default_rng(20240607)
    ns = reference_namespace()
    body = assign_body()
    rpos, member = reference_set(rng)
    rNames = ["r%02d" % k for k in range(N_REF)]
    rr = distances(rpos, None, rng, True)
    ref_edges = oracle.generate_tuples(Model().assign(rr).astype(np.int32), -1, True, 0, 0).tolist()

    # the old cluster file: printClusters on the reference network, as a fit would have left it
    with tempfile.TemporaryDirectory() as tmp:
        g = _Graph()
        g.add_vertex(N_REF)
        g.add_edge_list(ref_edges)
        with contextlib.redirect_stderr(io.StringIO()):
            clustering, _ = ns["printClusters"](g, rNames, outPrefix=os.path.join(tmp, "fit"), write_unwords=False)
    assert len(set(clustering.values())) == len(SIZES), "the reference network does not have the planted clusters"
    old_csv = "Taxon,Cluster\n" + "".join("%s,%d\n" % (r, clustering[r]) for r in rNames)
    old_csv_large = "Taxon,Cluster\n" + "".join("%s,%d\n" % (r, clustering[r] + 100) for r in rNames)

    far, nov = (40 * T, 40 * T), (-20 * T, -20 * T)
    join = [CENTRES[k] for k in ("A", "A", "A", "B", "B", "C", "D", "H")]
    x, y = towards("A", "B", 0.3), towards("B", "A", 0.3)             # linked to A and to B, and to each other
    cases = [
        ("joint_linked", "joint", join + [mid("D", "E"), mid("F", "G", "H"), CENTRES["E"], CENTRES["F"]], {}),
        ("joint_linked_print_ref", "joint", join + [mid("D", "E"), mid("F", "G", "H"), CENTRES["E"], CENTRES["F"]],
         {"write_references": True}),
        ("joint_unlinked", "joint", join[:6] + [far, nov, (nov[0] + 0.5 * T, nov[1]), x, y, mid("D", "E")], {}),
        ("joint_unlinked_print_ref", "joint", join[:6] + [far, nov, (nov[0] + 0.5 * T, nov[1]), x, y, mid("D", "E")],
         {"write_references": True}),
        ("joint_chain_not_asked", "joint", join + [x, y, CENTRES["D"], CENTRES["G"]], {}),
        ("joint_query_query", "joint", join + [x, y, CENTRES["D"], CENTRES["G"]], {"update_db": True}),
        ("single_linked", "joint", [mid("A", "B")], {}),
        ("single_unlinked", "joint", [far], {}),
        ("qc_max_merge_1", "joint", join + [mid("D", "E"), mid("F", "G", "H"), CENTRES["E"], CENTRES["F"]],
         {"qc_dict": {"run_qc": True, "max_merge": 1, "betweenness": False}}),
        ("qc_max_merge_2", "joint", join + [mid("D", "E"), mid("F", "G", "H"), CENTRES["E"], mid("F", "G", "H")],
         {"qc_dict": {"run_qc": True, "max_merge": 2, "betweenness": False}}),
        ("qc_all_fail", "joint", [mid("F", "G", "H")] * 5, {"qc_dict": {"run_qc": True, "max_merge": 2,
                                                                      "betweenness": False}}),
        ("serial_small_ids", "serial", join + [far, nov, (nov[0] + 0.5 * T, nov[1]), CENTRES["G"]], {}),
        ("serial_large_ids", "serial", join + [far, nov, (nov[0] + 0.5 * T, nov[1]), CENTRES["G"]],
         {"old_csv": "large"}),
        ("serial_merged_name", "serial", join[:4] + [mid("D", "E"), far], {}),
        ("stable_core", "stable", join + [mid("D", "E"), mid("F", "G", "H"), far, x], {"stable": "core"}),
        ("stable_accessory", "stable", join + [mid("D", "E"), mid("F", "G", "H"), far, x], {"stable": "accessory"}),
    ]
    doc = {"x_max": X_MAX, "y_max": Y_MAX, "rNames": rNames, "ref_edges": ref_edges, "old_csv": old_csv,
           "old_csv_large": old_csv_large, "planted": member, "cases": []}
    arrays = {}
    for name, mode, qpos, options in cases:
        csv = old_csv_large if options.get("old_csv") == "large" else old_csv
        case, qr, qq = run_case(ns, body, name, mode, rNames, ref_edges, csv, qpos, rpos, rng, options)
        doc["cases"].append(case)
        arrays[name + "_qr"], arrays[name + "_qq"] = qr, qq
        e = case["expected"]
        print("%-26s exit %s error %s qq %s clusters %s" % (name, e["exit"], e["error"], e["qq_shape"],
                                                          e["clustering"] and sorted(set(map(str, e["clustering"].values())))))
        print("    " + e["stderr"].replace("\n", "\n    "))
    with open(os.path.join(HERE, "assign.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "assign.npz"), **arrays)


if __name__ == "__main__":
    main()
