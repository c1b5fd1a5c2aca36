"""Writes tests/golden/rand.npz: small labeling pairs with what sklearn 1.7.2 gives for them
(pair_confusion_matrix, rand_score, adjusted_rand_score) and what the reference's
scripts/poppunk_calculate_rand_indices.py gives (its rand_index_score, imported from the script), and the text that
script writes -- its output file, its stderr, its exit code -- when run as a subprocess on small clustering CSVs.

    python tests/golden/make_golden_rand.py

Run in the BUILD container only (needs the reference checkout, sklearn, pandas and scipy); the fixture it writes is
data (labelings, floats, the CSVs and the recorded text) and is committed, the reference is not.

Labeling pairs (`pair%d_true`, `pair%d_pred`; `pair%d_confusion`, `_rand`, `_ari`, `_ri`): the script's three perfect
cases (one cluster each, n clusters each, and n = 1), all-in-one against singletons, nested pairs, renamed labels, a
giant cluster with singletons, numbers with gaps, independent labelings (an adjusted index below zero among them).
Runs (`run_names`; per run `<name>_args` the file names after --input, `<name>_subset` the --subset file or "",
`<name>_out`, `<name>_err`, `<name>_code`); `file_names` / `file_texts` hold every file the runs read."""
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np
import sklearn
from sklearn.metrics import adjusted_rand_score, rand_score
from sklearn.metrics.cluster import pair_confusion_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("POPPUNK_REFERENCE", "/root/reference")
SCRIPT = os.path.join(REF, "scripts", "poppunk_calculate_rand_indices.py")


def labeling_pairs():
    rng = np.random.default_rng(20)
    n = 60
    fine = rng.integers(0, 12, n)
    giant = np.zeros(40, dtype=np.int64)
    giant[30:] = np.arange(1, 11)
    gaps = np.array([1, 5, 33])[rng.integers(0, 3, 33)]
    return [
        (np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)),
        (np.array([0, 0]), np.array([0, 1])),
        (np.zeros(7, dtype=np.int64), np.zeros(7, dtype=np.int64)),
        (np.arange(6), np.arange(6)[::-1].copy()),
        (np.zeros(9, dtype=np.int64), np.arange(9)),
        (np.array([0, 0, 0, 1, 1, 1, 1]), np.array([0, 0, 1, 1, 2, 2, 2])),
        (fine, fine // 3),                                        # nested: fine refines coarse
        (fine, (fine * 7 + 3) % 12),                              # the same partition under other names
        (giant, np.arange(40) % 2),
        (gaps, rng.integers(1, 4, 33)),
        (rng.integers(0, 5, 50), rng.integers(0, 7, 50)),
        (np.array([0, 1, 0, 1, 0, 1]), np.array([0, 0, 1, 1, 2, 2])),  # adjusted index below zero
        (rng.integers(0, 20, 300), rng.integers(0, 20, 300)),
        (rng.integers(0, 40, 5000), rng.integers(0, 300, 5000)),
    ]


def csv_text(names, clusters, extra=None):
    lines = ["Taxon,Cluster" + (",Other" if extra is not None else "")]
    for k, (name, c) in enumerate(zip(names, clusters)):
        lines.append("%s,%d" % (name, c) + (",%d" % extra[k] if extra is not None else ""))
    return "\n".join(lines) + "\n"


def files():
    rng = np.random.default_rng(21)
    names = ["sample_%03d" % k for k in range(40)]
    a = rng.integers(1, 6, 40)
    b = np.where(rng.random(40) < 0.8, a, rng.integers(1, 9, 40))
    d = (a + 1) // 2                                             # a refines d
    order_b = rng.permutation(40)
    keep_c = np.sort(rng.permutation(40)[:29])                   # c lacks eleven names and has three of its own
    names_c = [names[k] for k in keep_c] + ["other_%d" % k for k in range(3)]
    c = list(rng.integers(1, 5, 29)) + [9, 9, 10]
    order_c = rng.permutation(32)
    return {
        "a.csv": csv_text(names, a, extra=rng.integers(0, 100, 40)),
        "b.csv": csv_text([names[k] for k in order_b], b[order_b]),
        "c.csv": csv_text([names_c[k] for k in order_c], [c[k] for k in order_c]),
        "d.csv": '"Cluster","Taxon"\n' + "".join('%d,"%s"\n' % (d[k], names[k]) for k in range(40)),
        "e.csv": csv_text(["elsewhere_%d" % k for k in range(5)], [1, 1, 2, 2, 3]),
        "bad.csv": "Sample,Group\nsample_000,1\nsample_001,2\n",
        "subset.txt": "".join(names[k] + "\n" for k in (3, 1, 17, 22, 8, 30, 31, 39, 12, 5)) + "ghost_name\n",
    }


RUNS = [
    ("same_names", ["a.csv", "b.csv", "d.csv"], ""),
    ("same_names_subset", ["a.csv", "b.csv", "d.csv"], "subset.txt"),
    ("lacking_names", ["a.csv", "b.csv", "c.csv"], ""),
    ("misformatted_and_disjoint", ["a.csv", "bad.csv", "e.csv"], ""),
    ("missing_file", ["a.csv", "nowhere.csv", "b.csv"], ""),
]


def main():
    spec = importlib.util.spec_from_file_location("reference_rand_script", SCRIPT)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)                              # (its run is under __name__ == "__main__")
    out = {"sklearn_version": np.array(sklearn.__version__)}
    pairs = labeling_pairs()
    out["n_pairs"] = np.array(len(pairs))
    for k, (t, p) in enumerate(pairs):
        out["pair%d_true" % k], out["pair%d_pred" % k] = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
        out["pair%d_confusion" % k] = pair_confusion_matrix(t, p).astype(np.int64)
        out["pair%d_rand" % k] = np.array(rand_score(t, p), dtype=np.float64)
        out["pair%d_ari" % k] = np.array(adjusted_rand_score(t, p), dtype=np.float64)
        out["pair%d_ri" % k] = np.array(script.rand_index_score(t, p), dtype=np.float64)
    texts = files()
    out["file_names"] = np.array(list(texts))
    out["file_texts"] = np.array([texts[name] for name in texts])
    out["run_names"] = np.array([name for name, _, _ in RUNS])
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in texts.items():
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        for name, inputs, subset in RUNS:
            cmd = [sys.executable, SCRIPT, "--input", ",".join(inputs), "--output", name + ".out"]
            if subset:
                cmd += ["--subset", subset]
            done = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
            path = os.path.join(tmp, name + ".out")
            out[name + "_args"] = np.array(inputs)
            out[name + "_subset"] = np.array(subset)
            out[name + "_out"] = np.array(open(path).read() if os.path.exists(path) else "")
            out[name + "_err"] = np.array(done.stderr)
            out[name + "_code"] = np.array(done.returncode)
            print(name, done.returncode, repr(done.stderr))
            print(out[name + "_out"])
    np.savez_compressed(os.path.join(HERE, "rand.npz"), **out)


if __name__ == "__main__":
    main()
