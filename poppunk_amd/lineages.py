"""Lineages within every strain: `poppunk_lineages --create-db` (PopPUNK/lineages.py:156-326) with the model fits of
all strains taken in one pass over the resident distance matrix.

  * `fit_strain_lineages(dist, names, strain_of, ranks, ...)` : per strain a fitted `models.LineageRanks` -- array for
    array what `LineageRanks.fit` gives on that strain's pruned matrix -- its printClusters numbers per rank and the
    `overall_lineage` dict of createOverallLineage (PopPUNK/utils.py:491-506).  Two device calls for the neighbour
    lists and the rank prefixes of every strain (engine.strain_knn_dev, engine.strain_ranks_dev) and one
    engine.cluster_sweep_dev for the cluster numbers of every strain and rank.
  * `create_db(args)` / `main(argv)` : the script's --create-db mode with its flags, files, messages and exit codes:
    `python -m poppunk_amd.lineages --create-db <db> --db-scheme <pkl> --output <prefix> ...`.

Differences from the script, all deliberate:
  * the distances are the STORED matrix (`<db>/<db>.dists` or --distances, read through distfile.readPickle); the
    script recomputes every strain's distances from the sketches (pp_sketchlib.queryDatabase), which gives the same
    rows bit for bit when the matrix was computed from the same sketches with the same k-mer list.
  * "Maximum rank must be less than the number of samples: n" is checked for every strain before the device is
    touched and raises RuntimeError; the script raises it from inside its loop, files of earlier strains written.
  * the strains are read with the csv module (pandas is not a dependency): groups in string order, members in row
    order, names from the first column, as `pd.read_csv(..., dtype=str).groupby(col)` gives them; rows whose cluster
    cell is empty are dropped as pandas drops NaN keys.
  * printClusters iterates Python sets, so the reference's row order inside a lineage depends on the hash seed; here
    the rows of a lineage follow the strain's member list (as poppunk_amd.network.printClusters does).
Not mirrored: the `.gt` rank graphs (save_network, --write-networks), --query-db, the sketching flags (--gpu-sketch,
--strand-preserved, --min-kmer-count, --exact-count: accepted, unused by --create-db upstream too), a path from the
sketches without the stored matrix, and more than one GPU.

Parity: get_kNN_distances and lowerRank are C++ that cannot be built in this tree (Eigen is missing); the kernels
agree bit for bit with this library's existing mirrors of them (ppk_knn_dev, ppk_lower_rank), whose parity with the
reference is unpinned (include/ppk.h, "OUTSIDE SURVEY 8")."""
import argparse
import csv
import os
import pickle
import shutil
import sys
from collections import defaultdict

import numpy as np

from . import distfile, engine, models

DEFAULT_LINEAGE_RESOLUTION = models.EPSILON      # PopPUNK/__main__.py: the script's default --lineage-resolution


def createOverallLineage(rank_list, lineage_clusters):
    """PopPUNK/utils.py:491-506: {'Rank_<r>': {isolate: number}, ..., 'overall': {isolate: 'a-b-c'}}."""
    overall_lineages = {'Rank_' + str(rank): {} for rank in rank_list}
    overall_lineages['overall'] = {}
    for isolate in lineage_clusters[rank_list[0]].keys():
        for rank in rank_list:
            overall_lineages['Rank_' + str(rank)][isolate] = lineage_clusters[rank][isolate]
        overall_lineages['overall'][isolate] = '-'.join(str(lineage_clusters[rank][isolate]) for rank in rank_list)
    return overall_lineages


def isolateNameToLabel(names):
    """PopPUNK/utils.py:473-488."""
    return [name.split('/')[-1].replace('.', '_').replace(':', '').replace('(', '_').replace(')', '_')
            for name in names]


def write_lineage_csv(outfile, names, clustering, suffix='_Lineage'):
    """writeClusterCsv(outfile, names, names, clustering, 'phandango', None, suffix=suffix) (PopPUNK/plot.py:598-760):
    `id` and one `<type><suffix>` column per clustering, one row per name, as pandas' to_csv writes them."""
    first = next(iter(clustering))
    rows = []
    for name, label in zip(names, isolateNameToLabel(names)):
        if name not in clustering[first]:
            sys.stderr.write("Cannot find " + name + " in clustering\n")
            sys.exit(1)
        rows.append([label] + [clustering[cluster_type][name] for cluster_type in clustering])
    sys.stderr.write("Parsed data, now writing to CSV\n")
    with open(outfile, 'w', newline='') as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(['id'] + [cluster_type + suffix for cluster_type in clustering])
        out.writerows(rows)


def print_overall_clustering(overall_lineage, output, include_list):
    """PopPUNK/lineages.py:469-493: `id,Cluster,Rank_...,overall`, strains in dict order, isolates in each strain's."""
    include = set(include_list)
    ranks = list(overall_lineage[next(iter(overall_lineage))].keys())
    isolate_info = {}
    for strain in overall_lineage:
        for rank in ranks:
            for isolate, value in overall_lineage[strain][rank].items():
                if isolate in include:
                    if isolate in isolate_info:
                        isolate_info[isolate].append(str(value))
                    else:
                        isolate_info[isolate] = [str(strain), str(value)]
    with open(output, 'w') as out:
        out.write('id,Cluster,' + ','.join(ranks) + '\n')
        for isolate in isolate_info:
            out.write(isolate + ',' + ','.join(isolate_info[isolate]) + '\n')


def read_strains(clustering_file, col_name):
    """`pd.read_csv(file, dtype=str).groupby(col_name)` as (strain, member names) pairs: strains in string order,
    members in row order, names from the first column; rows with an empty cluster cell are dropped."""
    with open(clustering_file, newline='') as f:
        table = [row for row in csv.reader(f) if row]
    header = table[0]
    if col_name not in header:
        raise KeyError(col_name)
    at = header.index(col_name)
    groups = defaultdict(list)
    for row in table[1:]:
        if at < len(row) and row[at] != '':
            groups[row[at]].append(row[0])
    return [(strain, groups[strain]) for strain in sorted(groups)]


def _split(arrays, counts):
    ends = np.cumsum(counts)
    return [tuple(a[e - c:e] for a in arrays) for c, e in zip(counts, ends)]


def _device_fit(dist, n, members, seg_off, depth, col, ranks, reciprocal_only, count_unique_distances, epsilon,
                device_id=0):
    """Both device calls and the cluster sweep -> (per strain the (i, j, dist) neighbour lists, per strain and rank
    lowerRank's (i, j, dist), numbers int32 [n_ranks, m]: every strain's own printClusters numbers).  The host tests
    replace this function with the numpy model."""
    torch = engine._torch()
    if not getattr(dist, "is_cuda", False):
        dist = torch.as_tensor(np.ascontiguousarray(dist, dtype=np.float32), device="cuda:%d" % device_id)
    dev = dist.device
    members_t = torch.as_tensor(members, device=dev)
    oi, oj, od = engine.strain_knn_dev(dist, members_t, seg_off, depth, col)
    prefix, pi, pj, lv, sd = engine.strain_ranks_dev(oj, od, seg_off, depth, ranks, reciprocal_only,
                                                     count_unique_distances, epsilon)
    m, n_ranks = int(seg_off[-1]), len(ranks)
    clusters, _ = engine.cluster_sweep_dev(pi, pj, lv, m, n_ranks)
    numbers = engine.strain_cluster_numbers(clusters, seg_off).cpu().numpy()
    sizes = np.diff(seg_off)
    d_s = np.minimum(depth, sizes - 1)
    lists = _split((oi.cpu().numpy(), oj.cpu().numpy(), od.cpu().numpy()), sizes * d_s)
    per_rank = []
    if reciprocal_only:
        # the stream is in (position, place) order: the entries of level <= q are lowerRank's output for rank q
        seg_t = torch.as_tensor(seg_off, device=dev)
        strain = torch.searchsorted(seg_t, pi, right=True) - 1
        li, lj = pi - seg_t[strain], pj - seg_t[strain]
        for q in range(n_ranks):
            keep = lv <= q
            counts = torch.bincount(strain[keep], minlength=len(sizes)).cpu().numpy()
            per_rank.append(_split((li[keep].cpu().numpy(), lj[keep].cpu().numpy(), sd[keep].cpu().numpy()), counts))
    else:
        # rank q keeps the first prefix[q][g] entries of the row of position g
        row_len = torch.as_tensor(np.repeat(d_s, sizes), device=dev)
        row = torch.repeat_interleave(torch.arange(m, device=dev), row_len)
        start = torch.cumsum(row_len, 0) - row_len
        place = torch.arange(int(row.shape[0]), device=dev) - start[row]
        for q in range(n_ranks):
            keep = place < prefix[q][row]
            counts = np.add.reduceat(prefix[q].cpu().numpy().astype(np.int64), seg_off[:-1])
            per_rank.append(_split((oi[keep].cpu().numpy(), oj[keep].cpu().numpy(), od[keep].cpu().numpy()), counts))
    outputs = [[per_rank[q][s] for q in range(n_ranks)] for s in range(len(sizes))]
    return lists, outputs, numbers


def fit_strain_lineages(dist, names, strain_of, ranks, max_search_depth=10000, reciprocal_only=False,
                        count_unique_distances=False, lineage_resolution=DEFAULT_LINEAGE_RESOLUTION,
                        use_accessory=False, min_count=10, device_id=0):
    """dist: the float32 [n(n-1)/2, 2] matrix of `names` (a CUDA tensor is read where it is, a numpy array uploaded to
    device_id).
    strain_of: {strain: member names in the strain's local order} (or the pairs read_strains gives); strains of fewer
    than min_count members are left out.  Returns {strain: (model, lineage_clusters, overall_lineage)} in strain_of's
    order: a fitted models.LineageRanks (nn_dists and lower_rank_dists floored at 1e-10, as __save_sparse__ does),
    {rank: {name: number}} with each dict in printClusters' order (lineage 1's members first, each lineage's in local
    order), and createOverallLineage's dict for `ranks` in the order given."""
    rank_list = [int(r) for r in ranks]
    pairs = list(strain_of.items()) if hasattr(strain_of, "items") else list(strain_of)
    kept = [(strain, list(isolates)) for strain, isolates in pairs if len(isolates) >= min_count]
    proto = models.LineageRanks(rank_list, max_search_depth, reciprocal_only, count_unique_distances,
                                lineage_resolution, dist_col=1 if use_accessory else 0)
    for strain, isolates in kept:
        proto._search_depth(len(isolates))       # "Maximum rank must be less than the number of samples: n"
    if not kept:
        return {}
    index = {name: k for k, name in enumerate(names)}
    members = np.asarray([index[name] for _, isolates in kept for name in isolates], dtype=np.int64)
    seg_off = np.concatenate([[0], np.cumsum([len(isolates) for _, isolates in kept])]).astype(np.int64)
    n = len(names)
    if int(dist.shape[0]) != n * (n - 1) // 2:
        raise RuntimeError("the distance matrix does not hold the %d pairs of %d samples" % (n * (n - 1) // 2, n))
    lists, outputs, numbers = _device_fit(dist, n, members, seg_off, proto.max_search_depth, proto.dist_col,
                                          proto.ranks, proto.reciprocal_only, proto.count_unique_distances,
                                          lineage_resolution, device_id)
    fitted = {}
    for s, (strain, isolates) in enumerate(kept):
        n_s = len(isolates)
        model = models.LineageRanks(rank_list, max_search_depth, reciprocal_only, count_unique_distances,
                                    lineage_resolution, dist_col=proto.dist_col)
        li, lj, ld = lists[s]
        model.nn_dists = model._coo(ld, li, lj, n_s)
        for q, rank in enumerate(model.ranks):
            ri, rj, rd = outputs[s][q]
            model.lower_rank_dists[rank] = model._coo(rd, ri, rj, n_s)
        model.fitted = True
        lineage_clusters = {}
        for q, rank in enumerate(model.ranks):
            mine = numbers[q, seg_off[s]:seg_off[s + 1]]
            order = np.argsort(mine, kind="stable")
            lineage_clusters[rank] = {isolates[k]: int(mine[k]) for k in order}
        fitted[strain] = (model, lineage_clusters, createOverallLineage(rank_list, lineage_clusters))
    return fitted


def get_options(argv=None):
    parser = argparse.ArgumentParser(description="Lineages within the strains of a database, fitted on the device",
                                     prog="python -m poppunk_amd.lineages")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument('--create-db', type=str, default=None, help="strain database to fit lineages within")
    mode.add_argument('--query-db', type=str, default=None, help="not available in this package")
    parser.add_argument('--db-scheme', required=True, help="pickle describing the lineage databases (written)")
    parser.add_argument('--output', required=True, help="prefix of the combined <output>.csv")
    parser.add_argument('--model-dir', help="directory of the strain model, if not the database")
    parser.add_argument('--distances', help="prefix of the stored distances, if not <db>/<db>.dists")
    parser.add_argument('--external-clustering', default=None, help="CSV of strain definitions")
    parser.add_argument('--clustering-col-name', default="Cluster", help="its strain column [Cluster]")
    parser.add_argument('--lineage-db-prefix', default="strain", help="prefix of the per-strain directories")
    parser.add_argument('--write-networks', default=False, action='store_true', help="accepted; no .gt graphs here")
    parser.add_argument('--overwrite', default=False, action='store_true', help="replace existing output")
    parser.add_argument('--threads', default=1, type=int)
    parser.add_argument('--gpu-sketch', default=False, action='store_true')
    parser.add_argument('--gpu-dist', default=False, action='store_true')
    parser.add_argument('--gpu-graph', default=False, action='store_true')
    parser.add_argument('--deviceid', default=0, type=int, help="the GPU the matrix is uploaded to")
    kind = parser.add_mutually_exclusive_group(required=False)
    kind.add_argument('--core', action='store_true', default=False)
    kind.add_argument('--accessory', action='store_true', default=False)
    parser.add_argument('--strand-preserved', action='store_true', default=False)
    parser.add_argument('--min-kmer-count', type=int, default=0)
    parser.add_argument('--exact-count', action='store_true', default=False)
    parser.add_argument('--ranks', default="1,2,3", type=str, help="comma separated ranks [1,2,3]")
    parser.add_argument('--max-search-depth', type=int, default=10000)
    parser.add_argument('--use-accessory', action='store_true', default=False)
    parser.add_argument('--min-count', default=10, type=int, help="smallest strain that gets lineages [10]")
    parser.add_argument('--count-unique-distances', action='store_true', default=False)
    parser.add_argument('--reciprocal-only', action='store_true', default=False)
    parser.add_argument('--lineage-resolution', type=float, default=DEFAULT_LINEAGE_RESOLUTION)
    return parser.parse_args(argv)


def create_db(args):
    """PopPUNK/lineages.py:156-326; see the module docstring for what differs."""
    from .sketchdb import readDBParams
    if not args.overwrite:
        for path in (args.output + '.csv', args.db_scheme):
            if os.path.exists(path):
                sys.stderr.write('Output file ' + path + ' exists; use --overwrite to replace it\n')
                sys.exit(1)

    sys.stderr.write("Identifying strains in existing database\n")
    if args.model_dir is None:
        args.model_dir = args.create_db
    if args.external_clustering is None:
        clustering_file = os.path.join(args.model_dir, os.path.basename(args.model_dir) + '_clusters.csv')
    else:
        clustering_file = args.external_clustering
    strains = read_strains(clustering_file, args.clustering_col_name)

    sys.stderr.write("Extracting properties of database\n")
    if args.distances is None:
        distances = os.path.join(args.create_db, os.path.basename(args.create_db) + ".dists")
    else:
        distances = args.distances
    kmers, sketch_sizes, codon_phased = readDBParams(args.create_db)
    rank_list = [int(x) for x in args.ranks.split(',')]
    if args.max_search_depth is not None:
        if args.max_search_depth <= max(rank_list):
            sys.stderr.write("Max search depth must be greater than the highest lineage rank\n")
            sys.exit(1)
        max_search_depth = args.max_search_depth
    else:
        max_search_depth = max(rank_list) * 10

    sys.stderr.write("Generating databases for individual strains\n")
    rlist, _, _, X = distfile.readPickle(distances, enforce_self=True, distances=True)
    fitted = fit_strain_lineages(X, rlist, strains, rank_list, max_search_depth, args.reciprocal_only,
                                 args.count_unique_distances, args.lineage_resolution, args.use_accessory,
                                 args.min_count, args.deviceid)
    all_isolates, lineage_dbs, overall_lineage = [], {}, {}
    isolate_list = []
    for strain, isolate_list in strains:
        sys.stderr.write("Making database for strain " + str(strain) + "\n")
        strain_db_name = args.lineage_db_prefix + '_' + str(strain) + '_lineage_db'
        if len(isolate_list) < args.min_count:
            continue
        lineage_dbs[strain] = strain_db_name
        all_isolates.extend(isolate_list)
        if os.path.isdir(strain_db_name) and args.overwrite:
            sys.stderr.write("--overwrite means {strain_db_name} will be deleted now\n")       # (the script's text)
            shutil.rmtree(strain_db_name)
        if not os.path.isdir(strain_db_name):
            try:
                os.makedirs(strain_db_name)
            except OSError:
                sys.stderr.write("Cannot create output directory " + strain_db_name + "\n")
                sys.exit(1)
        src_db = os.path.join(args.create_db, os.path.basename(args.create_db) + '.h5')
        dest_db = os.path.join(strain_db_name, os.path.basename(strain_db_name) + '.h5')
        rel_path = os.path.relpath(src_db, os.path.dirname(dest_db))
        if os.path.exists(dest_db) and args.overwrite:
            sys.stderr.write("--overwrite means {dest_db} will be deleted now\n")
            shutil.rmtree(dest_db)
        elif not os.path.exists(dest_db):
            os.symlink(rel_path, dest_db)
        distfile.storePickle(isolate_list, isolate_list, True, None, os.path.join(strain_db_name, strain_db_name + '.dists'))
        model, lineage_clusters, overall_lineage[strain] = fitted[strain]
        for rank in rank_list:
            n_clusters = max(lineage_clusters[rank].values())
            sys.stderr.write("Network for rank " + str(rank) + " has " + str(n_clusters) + " lineages\n")
        write_lineage_csv(os.path.join(strain_db_name, os.path.basename(strain_db_name) + '_lineages.csv'),
                          isolate_list, overall_lineage[strain])
        model.save(strain_db_name)

    print_overall_clustering(overall_lineage, args.output + '.csv', all_isolates)
    with open(args.db_scheme, 'wb') as pickle_file:
        pickle.dump([args.create_db, isolate_list, args.model_dir, clustering_file, args.clustering_col_name,
                     distances, kmers, sketch_sizes, codon_phased, max_search_depth, rank_list, args.use_accessory,
                     args.min_count, args.count_unique_distances, args.reciprocal_only, args.strand_preserved,
                     args.core, args.accessory, lineage_dbs], pickle_file)


def main(argv=None):
    args = get_options(argv)
    if args.create_db is not None:
        create_db(args)
    else:
        sys.stderr.write("--query-db is not available in poppunk_amd.lineages\n")
        sys.exit(1)


if __name__ == '__main__':
    main()
    sys.exit(0)
