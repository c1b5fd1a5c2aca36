"""The mandrake embedding behind poppunk_visualise's Microreact output (PopPUNK/mandrake.py), on the device.

generate_embedding mirrors PopPUNK/mandrake.py:22-120: the k nearest accessory neighbours of every sample
(poppunk_refine.get_kNN_distances), the stochastic cluster embedding of those lists (ppk_embed, DESIGN.md 3.11, in
place of SCE.wtsne / wtsne_gpu_fp32) and the same .dot file.  generate_embedding_from_sketches takes the neighbours
straight from the resident sketches (engine.knn_from_sketches, dist_col=1), so no n x n matrix exists."""
import os
import random
import sys

import numpy as np

from . import engine
from . import poppunk_refine


def _embedding_file(outPrefix, perplexity):
    return outPrefix + "/" + os.path.basename(outPrefix) + "_perplexity" + str(perplexity) + "_accessory_mandrake.dot"


def _seed(seed):
    if seed is None:        # as PopPUNK/mandrake.py:71-72 draws it
        random.Random()
        seed = random.randint(0, 2**32)
    return int(seed)


def write_dot(seqLabels, embedding, filename):
    """The .dot text of PopPUNK/mandrake.py:113-118: each label at 5 * its coordinates, Python's str(float)."""
    with open(filename, 'w') as nFile:
        nFile.write("graph G { ")
        for s, seqLabel in enumerate(seqLabels):
            nFile.write(f'"{seqLabel}"[x="{str(5*float(embedding[s][0]))}",y="{str(5*float(embedding[s][1]))}"]; ')
        nFile.write("}\n")


def generate_embedding(seqLabels, accMat, perplexity, outPrefix, overwrite, kNN=50,
                       maxIter=10000000, n_threads=1, use_gpu=False, device_id=0, seed=None):
    """PopPUNK/mandrake.py:generate_embedding: the 2-D embedding of the accessory distances of the n x n float32
    matrix accMat, written as outPrefix/<base>_perplexity<p>_accessory_mandrake.dot; returns that file name.
    use_gpu is accepted and ignored (this is the device path either way); n_threads only reaches the neighbour
    search.  seed: the generator's seed (None: drawn as the reference draws it)."""
    mandrake_filename = _embedding_file(outPrefix, perplexity)
    if os.path.isfile(mandrake_filename) and not overwrite:
        sys.stderr.write("Mandrake analysis already exists; add --overwrite to replace\n")
        return mandrake_filename
    sys.stderr.write("Running mandrake\n")
    kNN = min(kNN, len(seqLabels) - 1)
    I, J, dists = poppunk_refine.get_kNN_distances(accMat, kNN, 1, n_threads)
    _, embedding = engine.embed(I, J, dists, len(seqLabels), _seed(seed), perplexity=perplexity, max_iter=maxIter,
                                device_id=device_id)
    write_dot(seqLabels, embedding, mandrake_filename)
    return mandrake_filename


def embed_sketches(db, kmers, random_tbl, perplexity, kNN=50, maxIter=10000000, seed=None, random_correct=True,
                   method="auto"):
    """Sketches -> accessory neighbours -> Y, on the device: a float64 [n, 2] CUDA tensor."""
    kNN = min(kNN, db.n - 1)
    i, j, d = engine.knn_from_sketches(db, kmers, random_tbl, kNN, dist_col=1, random_correct=random_correct,
                                       method=method)
    P = engine.embed_weights_dev(i, j, d, db.n, perplexity)
    return engine.embed_dev(i, j, P, db.n, _seed(seed), max_iter=maxIter)


def generate_embedding_from_sketches(db, kmers, random_tbl, seqLabels, perplexity, outPrefix, overwrite, kNN=50,
                                     maxIter=10000000, seed=None, random_correct=True):
    """generate_embedding with the neighbours taken from the resident sketches (engine.SketchDB `db`) by
    engine.knn_from_sketches(..., dist_col=1): its "tiles" path for kNN <= 32, otherwise the square or bands path."""
    mandrake_filename = _embedding_file(outPrefix, perplexity)
    if os.path.isfile(mandrake_filename) and not overwrite:
        sys.stderr.write("Mandrake analysis already exists; add --overwrite to replace\n")
        return mandrake_filename
    sys.stderr.write("Running mandrake\n")
    Y = embed_sketches(db, kmers, random_tbl, perplexity, kNN, maxIter, seed, random_correct)
    write_dot(seqLabels, np.asarray(Y.cpu()), mandrake_filename)
    return mandrake_filename
