"""The golden case of the lineages within every strain (tests/golden/make_golden_lineages.py: the reference's own
create_db, LineageFit, createOverallLineage, print_overall_clustering, writeClusterCsv, storePickle and printClusters,
run unmodified on a known matrix) against poppunk_amd.lineages.create_db, shared by the host test (the numpy model in
the device's place) and the GPU test.

Every file is compared byte for byte or array for array, with one exception the reference forces: printClusters fills
its dict by iterating Python sets of names, so inside one lineage of the first rank the rows of the combined CSV come
in an order that depends on the interpreter's hash seed.  The combined CSV is therefore compared as its header and its
sequence of (strain, first-rank lineage) blocks, each block as a set of rows; poppunk_amd writes a block's rows in the
strain's member order."""
import json
import os
import pickle

import numpy as np
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    with open(os.path.join(HERE, "golden", "lineages_csv.json")) as f:
        texts = json.load(f)
    return texts, np.load(os.path.join(HERE, "golden", "lineages.npz"))


def blocks(csv_text):
    lines = csv_text.splitlines()
    out = []
    for line in lines[1:]:
        key = tuple(line.split(",")[1:3])
        if not out or out[-1][0] != key:
            out.append((key, set()))
        assert line not in out[-1][1]
        out[-1][1].add(line)
    return lines[0], out


def run_and_check(tmp_path, run, capsys):
    from poppunk_amd import lineages
    texts, arrays = load()
    rec = texts["runs"][run]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        os.makedirs("db")
        with open(os.path.join("db", "db_clusters.csv"), "w") as f:
            f.write(texts["clusters_csv"])
        with open(os.path.join("db", "db.dists.pkl"), "wb") as f:
            pickle.dump([texts["names"], texts["names"], True], f)
        np.save(os.path.join("db", "db.dists.npy"), arrays["dist"])
        np.savez(os.path.join("db", "db.npz"), kmers=np.asarray(rec["scheme"][6]), sketchsize64=rec["scheme"][7])
        capsys.readouterr()
        lineages.main(rec["argv"])
        assert capsys.readouterr().err == rec["stderr"]
        with open("out.csv") as f:
            assert blocks(f.read()) == blocks(rec["out_csv"])
        with open("scheme.pkl", "rb") as f:
            scheme = pickle.load(f)
        assert [v.tolist() if isinstance(v, np.ndarray) else v for v in scheme] == rec["scheme"]
        assert isinstance(scheme[6], np.ndarray)
        for strain, want in rec["strains"].items():
            stem = os.path.join(want["db"], want["db"])
            assert sorted(os.listdir(want["db"])) == want["files"]
            with open(stem + "_lineages.csv") as f:
                assert f.read() == want["lineages_csv"], strain
            with open(stem + "_fit.pkl", "rb") as f:
                assert pickle.load(f) == want["fit_pkl"]
            with open(stem + ".dists.pkl", "rb") as f:
                assert pickle.load(f) == want["names_pkl"]
            assert os.readlink(stem + ".h5") == want["h5_link"]
            files = [("nn", stem + "_sparse_dists.npz")] + [("rank%d" % r, stem + "_rank_%d_fit.npz" % r)
                                                            for r in want["fit_pkl"][0][0]]
            for what, path in files:
                m = scipy.sparse.load_npz(path).tocoo()
                key = "%s_%s_%s_" % (run, strain, what)
                assert np.array_equal(m.row, arrays[key + "row"]) and np.array_equal(m.col, arrays[key + "col"]), key
                assert m.data.dtype == np.float32 and np.array_equal(m.data.view(np.uint32),
                                                                     arrays[key + "data"].view(np.uint32)), key
    finally:
        os.chdir(cwd)
