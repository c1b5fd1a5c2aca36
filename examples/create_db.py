#!/usr/bin/env python3
"""From assemblies to clusters with this repository alone:

  FASTA files + a list of them (name <TAB> file)               PopPUNK/utils.py:410-471
    -> PopPUNK.sketchlib.constructDatabase(...)   sketches      PopPUNK/sketchlib.py:348-434
    -> PopPUNK.sketchlib.queryDatabase(...)       (core, acc.)  PopPUNK/sketchlib.py:475-632
    -> a threshold boundary -> edge list -> clusters

The assemblies are synthetic: a few families of related genomes, each a mutated copy of its family's root, written as
two-contig FASTA files into a temporary directory.  [EXT] The sketch rule is this project's own: the
database made here is not bit-compatible with one pp-sketchlib wrote.

    python examples/create_db.py [n_genomes] [genome_length] [workdir]          # needs an MI355X
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import distfile, models, qc, sketchlib, synth  # noqa: E402


def write_fasta(path, contigs, width=60):
    with open(path, "w") as f:
        for i, codes in enumerate(contigs):
            f.write(">contig_%d\n" % (i + 1))
            text = "".join("ACGT"[c] for c in codes)
            for a in range(0, len(text), width):
                f.write(text[a:a + width] + "\n")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    length = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_create_db_")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)          # 13, 17, 21, 25, 29
    rng = np.random.Generator(np.random.PCG64(synth.DEFAULT_SEED))

    # 1. assemblies: families of 6, the roots 5 % apart from the species root, the members 0.2 % from their root
    species = rng.integers(0, 4, size=length, dtype=np.uint8)

    def mutate(codes, pi):
        out = codes.copy()
        hit = rng.random(length) < pi
        out[hit] = (out[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) % 4
        return out

    os.makedirs(os.path.join(work, "assemblies"), exist_ok=True)
    listing = os.path.join(work, "assemblies.txt")
    family = []
    with open(listing, "w") as rfile:
        for i in range(n):
            if i % 6 == 0:
                root = mutate(species, 0.05)
            genome = mutate(root, 0.002)
            path = os.path.join(work, "assemblies", "genome_%03d.fa" % i)
            write_fasta(path, [genome[:length // 3], genome[length // 3:]])
            rfile.write("genome_%03d\t%s\n" % (i, path))
            family.append(i // 6)

    # 2. the sketch database: what `poppunk --create-db` starts with
    db_prefix = os.path.join(work, "example_db")
    names = sketchlib.constructDatabase(listing, kmers, 10000, db_prefix, threads=4, overwrite=True,
                                        strand_preserved=False, min_count=0, use_exact=False)
    ks, s64, _ = sketchlib.readDBParams(db_prefix)
    lengths, ambiguous = sketchlib.get_database_statistics(db_prefix)
    print("database: %d samples, k = %s, sketchsize64 = %d, mean length %.0f" % (len(names), ks.tolist(), s64, np.mean(lengths)))
    kept, failed = qc.sketchlibAssemblyQC(db_prefix, names, {"upper_n": None, "prop_n": 0.1, "length_sigma": 5,
                                                             "length_range": [None, None]})
    assert kept == names and not failed

    # 3. all-vs-all core / accessory distances
    X = sketchlib.queryDatabase(names, names, db_prefix, db_prefix, kmers, self=True)
    assert X.shape == (n * (n - 1) // 2, 2)
    same = np.asarray([family[i] == family[j] for i in range(n) for j in range(i + 1, n)])
    print("core distance: %.4f within a family (made 0.004 apart), %.4f between (made about 0.1 apart)"
          % (X[same, 0].mean(), X[~same, 0].mean()))

    # 4. a core-distance threshold between the two (poppunk --fit-model threshold) -> edges -> clusters
    threshold = float(X[same, 0].max() + X[~same, 0].min()) / 2.0
    boundary = models.RefineBoundary.from_threshold(threshold)
    edges = np.asarray(boundary.edges(X), dtype=np.int64).reshape(-1, 2)
    n_clusters, labels = distfile.clusters_from_edges(n, edges)
    print("threshold %.4f: %d within-strain pairs -> %d clusters (%d families)"
          % (threshold, len(edges), n_clusters, len(set(family))))
    assert n_clusters == len(set(family))
    print("files in", work)


if __name__ == "__main__":
    main()
