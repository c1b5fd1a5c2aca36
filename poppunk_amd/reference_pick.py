"""`python -m poppunk_amd.reference_pick`: poppunk_references (PopPUNK/reference_pick.py) on the MI355X.

Takes poppunk_references' flags.  Reference genomes are picked from a fitted network by network.extractReferences
(DESIGN.md 3.25), and the database is cut down to them:

    <output>/<output>.refs              the reference names, one a line (network.writeReferences)
    <output>/<output>.refs_graph.npz    the network among the references: `edges` int64 [m, 2], `n_vertices`
    <output>/<output>.dists.pkl/.npy    the distances among the references (qc.prune_distance_matrix)
    <output>/<output>.h5                the sketches of the references (sketchdb.removeFromDB), with --ref-db
    <output>/<output>_fit.pkl, _fit.npz, _clusters.csv    copied from --model

`--network` names this project's own network file, an .npz holding `edges` (int64 [m, 2]) and `n_vertices`:
graph-tool's .gt and cugraph's files cannot be read here.  `--threads` and `--use-gpu` are accepted and ignored (the
pick always runs on the device).
"""
import argparse
import os
import sys
from shutil import copyfile

import numpy as np

from . import __version__


def get_parser():
    """poppunk_references' flags (PopPUNK/reference_pick.py:26-54), with this package's own help texts"""
    parser = argparse.ArgumentParser(prog='poppunk_references',
                                     description='Pick reference genomes from a fitted network and cut the database '
                                                 'down to them')
    files = parser.add_argument_group('Input files')
    files.add_argument('--network', required=True,
                       help='the network to pick from (required): an .npz with "edges" (int64 [m, 2]) and '
                            '"n_vertices", as written by this package; graph-tool and cugraph files cannot be read')
    files.add_argument('--distances', required=True,
                       help='prefix of the distances of the whole database, <prefix>.pkl and <prefix>.npy (required)')
    files.add_argument('--ref-db', help='directory of the sketch database to prune; without it no database is written')
    files.add_argument('--model', help='directory of the model fit, whose files are copied beside the references')
    files.add_argument('--clusters', default=None,
                       help='a cluster file to copy in place of the one in the model directory')
    parser.add_argument_group('Output options').add_argument('--output', required=True,
                                                             help='output directory and file prefix (required)')
    other = parser.add_argument_group('Other options')
    other.add_argument('--threads', default=1, type=int, help='accepted and ignored [default = 1]')
    other.add_argument('--use-gpu', default=False, action='store_true',
                       help='accepted and ignored: the pick always runs on the device')
    other.add_argument('--version', action='version', version='%(prog)s ' + __version__)
    return parser


def load_network_npz(path):
    """(edges int64 [m, 2], n_vertices) of a network file of this package"""
    with np.load(path, allow_pickle=False) as f:
        if "edges" not in f or "n_vertices" not in f:
            raise ValueError("%s: a network file holds 'edges' and 'n_vertices'" % path)
        return np.ascontiguousarray(f["edges"], dtype=np.int64).reshape(-1, 2), int(f["n_vertices"])


def save_network_npz(G, prefix, suffix):
    """G = (edges, n_vertices) -> <prefix>/<basename(prefix)><suffix>.npz; the file's name"""
    edges = G[0].cpu().numpy() if hasattr(G[0], "cpu") else np.asarray(G[0])
    name = os.path.join(prefix, os.path.basename(prefix) + suffix + ".npz")
    np.savez(name, edges=np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2), n_vertices=np.int64(G[1]))
    return name


def pick(args):
    from . import network, qc, sketchdb
    from .distfile import readPickle
    if not os.path.isdir(args.output):
        try:
            os.makedirs(args.output)
        except OSError:
            sys.stderr.write("Cannot create output directory\n")
            sys.exit(1)
    base = os.path.join(args.output, os.path.basename(args.output))
    refList, _, _, distMat = readPickle(args.distances, enforce_self=True)
    G = load_network_npz(args.network)
    sys.stderr.write("Network loaded: " + str(G[1]) + " samples\n")
    reference_indices, reference_names, _, G_ref = network.extractReferences(G, refList, args.output,
                                                                             threads=args.threads,
                                                                             use_gpu=args.use_gpu)
    save_network_npz(G_ref, args.output, ".refs_graph")

    kept = frozenset(reference_names)
    names_to_remove = [name for name in refList if name not in kept]
    if names_to_remove:
        qc.prune_distance_matrix(refList, names_to_remove, distMat, base + ".dists")
        if args.ref_db is not None:
            sketchdb.removeFromDB(args.ref_db, args.output, names_to_remove)
            if os.path.exists(base + ".h5"):
                sys.stderr.write("Sketch DB exists in " + args.output + "\n"
                                 "Not overwriting. Output DB is: " + base + ".tmp.h5\n")
            else:
                os.rename(base + ".tmp.h5", base + ".h5")
    else:
        sys.stderr.write("No sequences to remove\n")

    if args.model is not None and os.path.isdir(args.model):
        sys.stderr.write("Copying model fit into " + args.output + "\n")
        model_base = os.path.join(args.model, os.path.basename(args.model))
        for ending in ("_fit.pkl", "_fit.npz"):
            copyfile(model_base + ending, base + ending)
        copyfile(args.clusters if args.clusters is not None else model_base + "_clusters.csv", base + "_clusters.csv")
    return reference_indices


def main(argv=None):
    pick(get_parser().parse_args(argv))
    sys.exit(0)


if __name__ == "__main__":
    main()
