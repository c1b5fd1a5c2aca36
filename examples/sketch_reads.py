#!/usr/bin/env python3
"""Reads and assemblies in one sketch database:

  a genome -> simulated reads (30x, 100 bases, 1 % substitutions, both strands) as a gzip FASTQ file,
              its assembly and an assembly 2 % diverged as FASTA files
    -> pp_sketchlib.constructDatabase(..., min_count=3)   the reads through the count filter, the assemblies as before
    -> pp_sketchlib.queryDatabase(...)                    the reads' distance to their own assembly and to the other

Sketched as if they were contigs the reads would share few bins with their own assembly: every sequencing error makes
up to k k-mers that occur once, and they take the bin minima.  [EXT] The sketch rule and the count table are this
project's own: the database is not bit-compatible with one pp-sketchlib wrote.

    python examples/sketch_reads.py [genome_length] [coverage] [workdir]          # needs an MI355X
"""
import gzip
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import pp_sketchlib, sketchdb, sketching, synth  # noqa: E402


def simulate_reads(rng, genome, coverage, read_len=100, error=0.01):
    n_reads = int(round(coverage * len(genome) / read_len))
    starts = rng.integers(0, len(genome), size=n_reads)
    reads = genome[(starts[:, None] + np.arange(read_len)[None, :]) % len(genome)]      # (a circular genome)
    hit = rng.random(reads.shape) < error
    reads[hit] = (reads[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) % 4
    flip = rng.random(n_reads) < 0.5
    reads[flip] = 3 - reads[flip][:, ::-1]
    return reads


def main():
    length = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    coverage = float(sys.argv[2]) if len(sys.argv) > 2 else 30.0
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ppk_sketch_reads_")
    kmers = [int(k) for k in synth.DEFAULT_KMERS]                     # 13, 17, 21, 25, 29
    rng = np.random.Generator(np.random.PCG64(synth.DEFAULT_SEED))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)

    genome = rng.integers(0, 4, size=length, dtype=np.uint8)
    other = genome.copy()
    hit = rng.random(length) < 0.02
    other[hit] = (other[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) % 4
    os.makedirs(work, exist_ok=True)
    files = [os.path.join(work, f) for f in ("reads.fastq.gz", "own.fa", "diverged.fa")]
    reads = simulate_reads(rng, genome, coverage)
    with gzip.open(files[0], "wb", compresslevel=1) as f:
        for i, r in enumerate(reads):
            f.write(b"@read_%d\n" % i + letters[r].tobytes() + b"\n+\n" + b"I" * len(r) + b"\n")
    for path, g in ((files[1], genome), (files[2], other)):
        with open(path, "wb") as f:
            f.write(b">contig_1\n" + letters[np.concatenate([g, g[:kmers[-1] - 1]])].tobytes() + b"\n")
    names = ["reads", "own_assembly", "diverged_assembly"]

    db = os.path.join(work, "reads_db", "reads_db")
    pp_sketchlib.constructDatabase(db, names, files, kmers, 10000, min_count=3, num_threads=3, calc_random=True)
    path, _ = pp_sketchlib._db_path(db)
    loaded = sketchdb.load(db, names, kmers)
    print("database %s: reads flags %s" % (path, sketchdb.reads_flags(path, names)))
    print("lengths: reads %d (estimated from %d read bases), assemblies %d and %d"
          % (loaded.lengths[0], reads.size, loaded.lengths[1], loaded.lengths[2]))
    X = pp_sketchlib.queryDatabase(db, db, names, names, kmers, random_correct=True)
    print("core distance of the reads to their own assembly  %.5f" % X[0, 0])
    print("core distance of the reads to the diverged one    %.5f   (the assemblies: %.5f, made 0.02 apart)" % (X[1, 0], X[2, 0]))
    assert X[0, 0] < 0.005 and X[0, 0] < X[1, 0] and abs(X[1, 0] - X[2, 0]) < 0.01

    # the same reads sketched as if they were contigs (min_count 1 admits every k-mer): the errors take the bins
    raw = sketching.sketch_files(["reads"], [files[0]], kmers, 10000, min_count=1)[0]
    filtered, assembly = loaded.sketches[0], loaded.sketches[1]

    def equal_bins(a, b):      # a bin is equal when none of its 14 bit planes differs
        diff = np.bitwise_or.reduce((a ^ b).reshape(len(kmers), -1, 14), axis=2)
        return 1.0 - sum(bin(int(x)).count("1") for x in diff.ravel()) / (64.0 * diff.size)

    print("bins equal to the assembly's: %.3f with min_count 3, %.3f with every k-mer admitted"
          % (equal_bins(filtered, assembly), equal_bins(raw[0], assembly)))
    print("files in", work)


if __name__ == "__main__":
    main()
