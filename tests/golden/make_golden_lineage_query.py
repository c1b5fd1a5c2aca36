#!/usr/bin/env python3
"""Generates tests/golden/lineage_query.npz and tests/golden/lineage_query.json: what the reference's own Python gives
for `poppunk_lineages --query-db` once the queries have their strains, on the case of make_golden_lineages.py.

Run in the BUILD container only (needs the reference checkout, networkx, pandas and scipy); what it writes is data
(query distance matrices of this generator's making, name lists, a placing, COO arrays, dicts, CSV and stderr texts)
and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast` and run unmodified), beyond make_golden_lineages.py's:
  PopPUNK/assign.py     the `if model.type == 'lineage':` block of assign_query_hdf5 (:528-573), its statements wrapped
                        in a function of the names they read
  PopPUNK/lineages.py   query_db from the statement after its first assign_query_hdf5 call to its end (:416-466),
                        wrapped likewise; print_overall_clustering
  PopPUNK/models.py     loadClusterFit, LineageFit.extend, LineageFit.load, reduce_rank
  PopPUNK/utils.py      createOverallLineage;   PopPUNK/plot.py  writeClusterCsv;   PopPUNK/network.py  printClusters
Stand-ins: make_golden_lineages.py's; poppunk_refine.extend is oracle.extend (the C++ cannot be built here);
queryDatabase slices the two query matrices; addRandom does nothing; the per-strain assign_query_hdf5 that query_db's
tail calls loads the strain's model with loadClusterFit (its two messages not recorded) and runs the extracted block.
The strain databases come from the reference's create_db, run here as make_golden_lineages.py runs it.

The case: make_golden_lineages.py's n = 300 matrix and strains; 30 queries, each placed on a template member t of a
strain: its distances are t's, some moved by multiples of 2^-12.  q00 .. q03 are identical to their template (distance
0 to it, the floor in the model: ties across the two sides), q04 and q05 are identical to each other, q06 sits in a
strain below --min-count, q07 in a strain number no reference has."""
import ast
import contextlib
import io
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_lineages as mgl         # noqa: E402
import make_golden_network as mgn          # noqa: E402
from oracle import oracle                  # noqa: E402

REF = mgn.REF
N, N_QRY = mgl.N, 30


def long_index(a, b, n):
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * (2 * n - lo - 1) // 2 + (hi - lo - 1)


def the_queries(dist, numbers):
    """(qr [N_QRY * N, 2], qq long form, template of every query, strain text of every query)"""
    rng = np.random.default_rng(77)
    sizes = np.bincount(numbers)
    big = [s for s in range(1, len(sizes)) if sizes[s] >= mgl.MIN_COUNT]
    small = [s for s in range(1, len(sizes)) if 2 <= sizes[s] < mgl.MIN_COUNT]
    strain = [big[k % len(big)] for k in range(N_QRY)]
    strain[4] = strain[5]
    strain[6] = small[0]
    template = np.asarray([rng.choice(np.flatnonzero(numbers == s)) for s in strain])
    template[5] = template[4]
    step = 2.0 ** -12

    def row_to(t, others, noisy):
        d = np.where((others == t)[:, None], 0.0, dist[long_index(t, np.where(others == t, (t + 1) % N, others), N)])
        if noisy:
            d = d + step * rng.integers(0, 3, d.shape)
        return d.astype(np.float32)
    refs = np.arange(N)
    qr = np.zeros((N_QRY * N, 2), dtype=np.float32)
    for q in range(N_QRY):
        qr[q * N:(q + 1) * N] = row_to(template[q], refs, noisy=q >= 6)
    qr[5 * N:6 * N] = qr[4 * N:5 * N]
    a, b = np.triu_indices(N_QRY, 1)
    same = template[a] == template[b]
    qq = np.where(same[:, None], step * rng.integers(1, 4, (len(a), 2)),
                  dist[long_index(template[a], np.where(same, (template[b] + 1) % N, template[b]), N)]).astype(np.float32)
    qq[long_index(4, 5, N_QRY)] = 0.0
    for k in np.flatnonzero(b == 5):                     # q05's distances are q04's
        if a[k] < 4:
            qq[k] = qq[long_index(a[k], 4, N_QRY)]
    for k in np.flatnonzero(a == 5):
        qq[k] = qq[long_index(4, b[k], N_QRY)]
    texts = [str(s) for s in strain]
    texts[7] = str(len(sizes) + 5)
    return qr, qq, template, texts


def wrap(statements, name, args):
    fn = ast.FunctionDef(name=name, args=ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in args],
                                                        kwonlyargs=[], kw_defaults=[], defaults=[]),
                         body=statements, decorator_list=[], type_params=[])
    return ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))


def function_of(path, name):
    tree = ast.parse(open(path).read())
    return next(node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == name)


def add_reference_pieces(ns):
    path = os.path.join(REF, "PopPUNK", "assign.py")
    fn = function_of(path, "assign_query_hdf5")
    block = next(node for node in ast.walk(fn)
                 if isinstance(node, ast.If) and ast.unparse(node.test) == "model.type == 'lineage'" and
                 any("extend" in ast.unparse(stmt) for stmt in node.body))
    body = block.body + [ast.Return(value=ast.Name(id="isolateClustering", ctx=ast.Load()))]
    exec(compile(wrap(body, "lineage_branch", ["model", "output", "rNames", "qNames", "qrDistMat", "kmers",
                                               "strand_preserved", "overwrite", "threads", "gpu_dist", "gpu_graph",
                                               "graph_weights"]), path, "exec"), ns)
    path = os.path.join(REF, "PopPUNK", "lineages.py")
    fn = function_of(path, "query_db")
    first = next(k for k, stmt in enumerate(fn.body) if isinstance(stmt, ast.Assign) and
                 ast.unparse(stmt.targets[0]) == "isolateClustering")
    body = fn.body[first + 1:] + [ast.Return(value=ast.Name(id="overall_lineage", ctx=ast.Load()))]
    exec(compile(wrap(body, "query_db_tail", ["args", "isolateClustering", "qNames", "lineage_dbs", "rank_list", "core",
                                              "accessory", "strand_preserved", "dbFuncs", "qc_dict"]), path, "exec"), ns)
    mgn.extract_functions(os.path.join(REF, "PopPUNK", "models.py"), ["loadClusterFit"], ns)


def main():
    import re
    dist, numbers, names, order = mgl.the_case()
    qr, qq, template, strain_text = the_queries(dist, numbers)
    qnames = ["queries/q%02d.fa" % k for k in range(N_QRY)]
    q_index = {name: k for k, name in enumerate(qnames)}
    r_index = {name: k for k, name in enumerate(names)}
    ns = mgl.reference_namespace(dist, names)
    ns["re"] = re
    ns["poppunk_refine"].extend = staticmethod(
        lambda mat, qq_sq, qr_rect, knn, threads: oracle.extend(mat[0], mat[1], mat[2], qq_sq, qr_rect, knn))
    square = ns["pp_sketchlib"].longToSquare
    ns["pp_sketchlib"].longToSquare = staticmethod(
        lambda distVec, num_threads=1: square(distVec) if len(distVec) else np.zeros((1, 1), dtype=np.float32))
    ns["addRandom"] = lambda *a, **kw: None

    def query_database(rNames, qNames, dbPrefix, queryPrefix, klist, self, number_plot_fits, threads, use_gpu):
        q = np.asarray([q_index[name] for name in qNames], dtype=np.int64)
        if self:
            a, b = np.triu_indices(len(q), 1)
            return np.ascontiguousarray(qq[long_index(q[a], q[b], N_QRY)]).reshape(-1, 2)
        r = np.asarray([r_index[name] for name in rNames], dtype=np.int64)
        return np.ascontiguousarray(qr[(q[:, None] * N + r[None, :]).ravel()])
    ns["queryDatabase"] = query_database
    add_reference_pieces(ns)
    recorded = {}

    def assign_query_hdf5(dbFuncs, ref_db, qNames, output, qc_dict, update_db, write_references, distances, serial,
                          stable, threads, overwrite, plot_fit, graph_weights, model_dir, strand_preserved,
                          previous_clustering, external_clustering, core, accessory, gpu_dist, gpu_graph,
                          save_partial_query_graph=False, use_full_network=True):
        stem = os.path.join(model_dir, os.path.basename(model_dir))
        with contextlib.redirect_stderr(io.StringIO()):
            model = ns["loadClusterFit"](stem + "_fit.pkl", stem + "_fit.npz")
        model.set_threads(threads)
        with open(distances + ".pkl", "rb") as f:
            rNames = pickle.load(f)[0]
        qrDistMat = query_database(rNames, qNames, ref_db, output, None, False, 0, threads, gpu_dist)
        clustering = ns["lineage_branch"](model, output, rNames, qNames, qrDistMat, None, strand_preserved, overwrite,
                                          threads, gpu_dist, gpu_graph, graph_weights)
        recorded[ref_db] = (model, rNames, list(qNames), clustering)
        return clustering
    ns["assign_query_hdf5"] = assign_query_hdf5

    arrays = {"qr": qr, "qq": qq, "template": template.astype(np.int64)}
    texts = {"qnames": qnames, "strain_of_query": dict(zip(qnames, strain_text)), "runs": {}}
    csv_text = "Taxon,Cluster\n" + "".join("%s,%d\n" % (names[k], numbers[k]) for k in order)
    isolate_clustering = {"combined": {names[k]: str(numbers[k]) for k in range(N)}}
    isolate_clustering["combined"].update(texts["strain_of_query"])
    cwd = os.getcwd()
    for run, flags in mgl.RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                os.makedirs("db")
                with open(os.path.join("db", "db_clusters.csv"), "w") as f:
                    f.write(csv_text)
                create_argv = ["poppunk_lineages", "--create-db", "db", "--db-scheme", "scheme.pkl", "--output", "out",
                               "--min-count", str(mgl.MIN_COUNT)] + flags
                old_argv, sys.argv = sys.argv, create_argv
                try:
                    with contextlib.redirect_stderr(io.StringIO()):
                        ns["create_db"](ns["get_options"]())
                finally:
                    sys.argv = old_argv
                with open("scheme.pkl", "rb") as f:
                    scheme = pickle.load(f)
                lineage_dbs, rank_list = scheme[18], scheme[10]
                query_argv = ["poppunk_lineages", "--query-db", "queries", "--db-scheme", "scheme.pkl", "--output",
                              "assigned"]
                sys.argv = query_argv
                try:
                    args = ns["get_options"]()
                finally:
                    sys.argv = old_argv
                os.makedirs("assigned")
                recorded.clear()
                err = io.StringIO()
                with contextlib.redirect_stderr(err):
                    overall = ns["query_db_tail"](args, isolate_clustering, qnames, lineage_dbs, rank_list, scheme[16],
                                                  scheme[17], scheme[15], {}, {"run_qc": False})
                rec = {"create_argv": create_argv[1:], "argv": query_argv[1:], "stderr": err.getvalue(),
                       "out_csv": open("assigned.csv").read(),
                       "lineages_csv": open(os.path.join("assigned", "assigned_lineages.csv")).read(),
                       "overall": {strain: {key: {name: value for name, value in d.items()}
                                            for key, d in overall[strain].items()} for strain in overall},
                       "strains": {}}
                for strain, db_name in lineage_dbs.items():
                    if db_name not in recorded:
                        continue
                    model, r_names, q_names, clustering = recorded[db_name]
                    rec["strains"][strain] = {"rNames": r_names, "qNames": q_names,
                                              "clusters": {str(rank): {name: int(v) for name, v in clustering[rank].items()}
                                                           for rank in model.ranks}}
                    for what, m in [("nn", model.nn_dists)] + [("rank%d" % r, model.lower_rank_dists[r])
                                                               for r in model.ranks]:
                        m = m.tocoo()
                        key = "%s_%s_%s_" % (run, strain, what)
                        arrays[key + "row"], arrays[key + "col"] = m.row.astype(np.int64), m.col.astype(np.int64)
                        arrays[key + "data"] = m.data.astype(np.float32)
                texts["runs"][run] = rec
            finally:
                os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, "lineage_query.npz"), **arrays)
    with open(os.path.join(HERE, "lineage_query.json"), "w") as f:
        json.dump(texts, f, indent=1)
    print({run: (sorted(rec["strains"]), len(rec["out_csv"].splitlines())) for run, rec in texts["runs"].items()})


if __name__ == "__main__":
    main()
