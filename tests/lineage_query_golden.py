"""The golden case of the query batch added to the lineages of every strain (tests/golden/make_golden_lineage_query.py:
the reference's own lineage block of assign_query_hdf5, query_db's tail, LineageFit.extend, createOverallLineage,
print_overall_clustering and writeClusterCsv, run unmodified on known matrices) against
poppunk_amd.lineages.extend_strain_lineages and query_db, shared by the host test (the numpy model in the device's
place) and the GPU test.

The strain databases are written by this package's own --create-db on lineage_golden's case.  The two steps in front of
the lineages are taken from the record, as the generator takes them: the distances (lineages._query_distances) and the
strain of every query (lineages._assign_strains).  Files are compared byte for byte and arrays bit for bit, but for
what the reference's iteration of Python sets makes depend on the hash seed: the combined CSV is compared block by
block (lineage_golden.blocks) and the cluster dicts as dicts."""
import json
import os
import pickle

import numpy as np

import lineage_golden

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    with open(os.path.join(HERE, "golden", "lineage_query.json")) as f:
        texts = json.load(f)
    return texts, np.load(os.path.join(HERE, "golden", "lineage_query.npz"))


def run_and_check(tmp_path, run, capsys, monkeypatch):
    from poppunk_amd import lineages, models, sketchdb
    base_texts, base_arrays = lineage_golden.load()
    texts, arrays = load()
    rec = texts["runs"][run]
    names, qnames = base_texts["names"], texts["qnames"]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        os.makedirs("db")
        with open(os.path.join("db", "db_clusters.csv"), "w") as f:
            f.write(base_texts["clusters_csv"])
        with open(os.path.join("db", "db.dists.pkl"), "wb") as f:
            pickle.dump([names, names, True], f)
        np.save(os.path.join("db", "db.dists.npy"), base_arrays["dist"])
        scheme = base_texts["runs"][run]["scheme"]
        np.savez(os.path.join("db", "db.npz"), kmers=np.asarray(scheme[6]), sketchsize64=scheme[7])
        lineages.main(rec["create_argv"])
        sketchdb.save_npz(os.path.join("queries", "queries"), qnames, scheme[6],
                          np.zeros((len(qnames), len(scheme[6]), 2), dtype=np.uint64), 2, 14)
        placing = {name: str(number) for name, number in zip(names, base_arrays["strain_numbers"])}
        placing.update(texts["strain_of_query"])
        monkeypatch.setattr(lineages, "_query_distances", lambda *a, **kw: (arrays["qr"], arrays["qq"]))
        monkeypatch.setattr(lineages, "_assign_strains", lambda *a, **kw: {"combined": placing})
        capsys.readouterr()
        lineages.main(rec["argv"])
        assert capsys.readouterr().err == rec["stderr"]
        with open("assigned.csv") as f:
            assert lineage_golden.blocks(f.read()) == lineage_golden.blocks(rec["out_csv"])
        with open(os.path.join("assigned", "assigned_lineages.csv")) as f:
            assert f.read() == rec["lineages_csv"]

        # the models and dicts behind the files
        with open("scheme.pkl", "rb") as f:
            lineage_dbs = pickle.load(f)[18]
        fitted = {strain: models.LineageRanks.load(lineage_dbs[strain]) for strain in rec["strains"]}
        names_of = {strain: rec["strains"][strain]["rNames"] for strain in rec["strains"]}
        got = lineages.extend_strain_lineages(fitted, names_of, qnames, texts["strain_of_query"], arrays["qr"],
                                              arrays["qq"], names)
        assert sorted(got) == sorted(rec["strains"])
        for strain, want in rec["strains"].items():
            model, clusters, overall = got[strain]
            assert [q for q in qnames if texts["strain_of_query"][q] == strain] == want["qNames"]
            files = [("nn", model.nn_dists)] + [("rank%d" % r, model.lower_rank_dists[r]) for r in model.ranks]
            for what, m in files:
                key = "%s_%s_%s_" % (run, strain, what)
                assert np.array_equal(m.row, arrays[key + "row"]) and np.array_equal(m.col, arrays[key + "col"]), key
                assert m.data.dtype == np.float32 and np.array_equal(m.data.view(np.uint32),
                                                                     arrays[key + "data"].view(np.uint32)), key
            assert {str(rank): d for rank, d in clusters.items()} == want["clusters"], strain
            assert overall == rec["overall"][strain], strain
    finally:
        os.chdir(cwd)
