"""Rand and adjusted Rand indices between PopPUNK clustering CSVs: the job of
scripts/poppunk_calculate_rand_indices.py, with the names matched through dictionaries and every pair of files that
compares the same samples taken in one device call.

    python -m poppunk_amd.rand_indices --input a.csv,b.csv,c.csv [--output rand.out] [--subset names.txt]

The output has the script's header and its seven tab-separated columns (File_1, File_2, n_1, n_2, n_compared,
Rand_index, Adjusted_Rand_index), pairs in input order with x < y, files keyed by basename, the two indices as str() of
the script's floats (poppunk_amd.scores restates them from the device's integer sums).
"""
import csv
import os
import sys

import numpy as np

from . import scores

HEADER = ["File_1", "File_2", "n_1", "n_2", "n_compared", "Rand_index", "Adjusted_Rand_index"]
ITEM_MESSAGE = "can only convert an array of size 1 to a Python scalar"


def read_clustering(path):
    """The Taxon and Cluster columns of a clustering CSV, found by header name: (names, clusters) as lists of the
    strings the file holds, or None when either column is missing.  ValueError for an empty or missing Cluster field
    (the script dies in np.bincount there)."""
    with open(path, newline="") as f:
        rows = csv.reader(f, quotechar='"')
        header = next(rows, None)
        if header is None or "Taxon" not in header or "Cluster" not in header:
            return None
        taxon, cluster = header.index("Taxon"), header.index("Cluster")
        names, clusters = [], []
        for line, row in enumerate(rows, start=2):
            if not row:
                continue
            if len(row) <= cluster or row[cluster] == "":
                raise ValueError("%s, line %d: empty Cluster field" % (path, line))
            names.append(row[taxon] if len(row) > taxon else "")
            clusters.append(row[cluster])
    return names, clusters


def _index(names):
    """{name: its row, or -1 where the file holds the name more than once}."""
    out = {}
    for k, name in enumerate(names):
        out[name] = -1 if name in out else k
    return out


def _item(index, name):
    """np.where(names == name)[0].item(): the row of a name held exactly once, the script's ValueError otherwise."""
    k = index.get(name, -1)
    if k < 0:
        raise ValueError(ITEM_MESSAGE)
    return k


def calculate_rand_indices(inputs, output="rand.out", subset=None, device_id=0):
    """scripts/poppunk_calculate_rand_indices.py with its arguments: `inputs` the clustering CSVs (a list, or the
    script's comma-separated string), `output` the table to write, `subset` a file of sample names, one per line, to
    restrict every comparison to.  The script's messages go to stderr in its words: a file without Taxon and Cluster
    columns is reported and left out; a file that does not exist ends the run with SystemExit(1); a subset name the
    first file of a pair lacks is reported ("Cannot find ... in both datasets"); a pair with nothing to compare is
    reported ("No overlapping sequences ...") and has no line.  ValueError where the script's .item() raises: a
    compared name that the first file of a pair holds twice, or a subset name that the first file has and the second
    lacks or holds twice.  Returns the rows written, as lists of seven strings.

    [EXT] Names and clusters are compared as the strings the files hold, as scores.read_cluster_csv does.  The script
    reads through pandas, which turns an all-numeric column into numbers: clusters "1" and "01" of such a column are
    one cluster there and two here, and an all-numeric Taxon column never matches the (string) lines of a subset file
    there.  pandas also reads "NA", "NaN" and their like as missing; here only an empty Cluster field is."""
    if isinstance(inputs, str):
        inputs = inputs.split(",")
    names_list, cluster_list = {}, {}
    for input_file in inputs:
        if os.path.isfile(input_file):
            parsed = read_clustering(input_file)
            if parsed is not None:
                bn = os.path.basename(input_file)
                names_list[bn], cluster_list[bn] = parsed
            else:
                sys.stderr.write("Input files need to be PopPUNK clustering CSVs; " + input_file +
                                 " appears to be misformatted\n")
        else:
            sys.stderr.write("File does not exist: " + input_file + "\n")
            raise SystemExit(1)
    subset_seq = []
    if subset is not None and os.path.isfile(subset):
        with open(subset, "r") as subset_file:
            subset_seq = [line.rstrip() for line in subset_file]

    # every pair's compared rows, in the script's order; its messages as it goes
    files = list(names_list)
    index = {bn: _index(names_list[bn]) for bn in files}
    pairs = []                                # (x, y, names compared, rows of x, rows of y)
    for x, input_x in enumerate(files):
        for input_y in files[x + 1:]:
            compared, rows_x, rows_y = [], [], []
            if subset is None:
                for i, name in enumerate(names_list[input_y]):
                    if name in index[input_x]:
                        rows_y.append(i)
                        rows_x.append(_item(index[input_x], name))
                        compared.append(name)
            else:
                for name in subset_seq:
                    if name in index[input_x]:
                        rows_y.append(_item(index[input_y], name))
                        rows_x.append(_item(index[input_x], name))
                        compared.append(name)
                    else:
                        sys.stderr.write("Cannot find " + name + " in both datasets")
            if rows_x:
                pairs.append((input_x, input_y, compared, rows_x, rows_y))
            else:
                sys.stderr.write("No overlapping sequences for files " + input_x + " and " + input_y + "\n")

    # the pairs that compare one set of samples (each once) share a device call: a level per file, every level
    # against every level
    groups = {}
    for k, (input_x, input_y, compared, _, _) in enumerate(pairs):
        key = frozenset(compared)
        groups.setdefault(key if len(key) == len(compared) else k, []).append(k)
    results = {}
    for members in groups.values():
        compared = pairs[members[0]][2]
        level_of, levels = {}, []
        if len(members) == 1:                 # (also the pair whose second file repeats a name: its rows as they are)
            input_x, input_y, _, rows_x, rows_y = pairs[members[0]]
            level_of = {input_x: 0, input_y: 1}
            levels = [scores.factorise([cluster_list[input_x][r] for r in rows_x])[0],
                      scores.factorise([cluster_list[input_y][r] for r in rows_y])[0]]
        else:
            for k in members:
                for bn in pairs[k][:2]:
                    if bn not in level_of:
                        level_of[bn] = len(levels)
                        levels.append(scores.factorise([cluster_list[bn][index[bn][name]] for name in compared])[0])
        sq, _, labels, _, sq_cells, _ = scores._device_sums(np.stack(levels), None, device_id)
        for k in members:
            lx, ly = level_of[pairs[k][0]], level_of[pairs[k][1]]
            results[k] = (len(compared), int(sq[lx]), int(sq[ly]), int(sq_cells[lx, ly]), int(labels[lx]),
                          int(labels[ly]))

    written = []
    with open(output, "w") as output_file:
        output_file.write("\t".join(HEADER) + "\n")
        for k, (input_x, input_y, _, rows_x, _) in enumerate(pairs):
            sums = results[k]
            ri = scores._rand_index(*sums)
            ari = scores._adjusted_rand(*sums[:4])
            row = [input_x, input_y, str(len(cluster_list[input_x])), str(len(cluster_list[input_y])),
                   str(len(rows_x)), str(ri), str(ari)]
            output_file.write("\t".join(row) + "\n")
            written.append(row)
    return written


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Calculate Rand index and adjusted Rand index between two clusterings",
                                     prog="calculate_rand_indices")
    parser.add_argument("--input", required=True, type=str,
                        help="Comma separated list of clustering CSVs between which indices should be calculated "
                             "(required)")
    parser.add_argument("--output", help="Name of output file [default = rand.out]", type=str, default="rand.out")
    parser.add_argument("--subset", type=str,
                        help="File with list of sequences to extract for comparison, one per line, no header; must be "
                             "present in all CSVs")
    parser.add_argument("--device", type=int, default=0, help="GPU to use (default = 0)")
    args = parser.parse_args(argv)
    calculate_rand_indices(args.input, args.output, args.subset, args.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
