"""Lineages within every strain: `poppunk_lineages --create-db` (PopPUNK/lineages.py:156-326) with the model fits of
all strains taken in one pass over the resident distance matrix.

  * `fit_strain_lineages(dist, names, strain_of, ranks, ...)` : per strain a fitted `models.LineageRanks` -- array for
    array what `LineageRanks.fit` gives on that strain's pruned matrix -- its printClusters numbers per rank and the
    `overall_lineage` dict of createOverallLineage (PopPUNK/utils.py:491-506).  Two device calls for the neighbour
    lists and the rank prefixes of every strain (engine.strain_knn_dev, engine.strain_ranks_dev) and one
    engine.cluster_sweep_dev for the cluster numbers of every strain and rank.
  * `create_db(args)` / `main(argv)` : the script's --create-db mode with its flags, files, messages and exit codes:
    `python -m poppunk_amd.lineages --create-db <db> --db-scheme <pkl> --output <prefix> ...`.
  * `extend_strain_lineages(fitted, names_of, qNames, strain_of_query, qr, qq, rNames)` : a query batch added to the
    lineage models of the strains it was assigned to (the lineage branch of assign_query_hdf5, PopPUNK/assign.py:
    528-573, per strain `LineageFit.extend`, lowerRank per rank and printClusters) in one pass over the resident
    query x reference and query x query matrices: engine.strain_extend_dev, engine.strain_ranks_dev
    and one engine.cluster_sweep_dev.
  * `query_db(args)` : the script's --query-db mode (PopPUNK/lineages.py:329-466) on loaded pieces:
    `python -m poppunk_amd.lineages --query-db <sketched query db> --db-scheme <pkl> --output <prefix>`; writes
    `<output>/<output>_lineages.csv` and `<output>.csv`.

Differences of --query-db from the script, all deliberate:
  * --query-db names an already SKETCHED query database, not a list of assemblies (sketching is out of scope), and
    addRandom is not called (INTEGRATION.md section 5's rule for query databases).
  * strain assignment goes through assign.assign_query_clusters in joint mode on the resident query x reference
    matrix; the strain network is represented by its components, read from `<model_dir>_clusters.csv` into
    ReferenceNetwork(..., labels=...) (`.gt` files cannot be read here; for a full network the clusters are the
    components, assign.py's exactness condition); the strain model comes through the from_npz loaders.
  * the query x query matrix is computed once for all queries, not per strain: the rows are the same.
  * a strain's queries are taken in the query database's order; the script takes them in the order its strain
    clustering dict lists them.  Only the order inside runs of equal distances can differ.
  * if no strain with a lineage database received a query the script dies on `list(overall_lineage.keys())[0]`;
    here that is a RuntimeError that says so.
  * `<output>/<output>_lineages.csv` is written once per strain to the same path, as the script does: the last
    strain's remains.

Differences of --create-db from the script, all deliberate:
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
Not mirrored: the `.gt` rank graphs (save_network, --write-networks), --update-db of lineage models (the extended
models are returned, not saved back), sketching the queries, the sketching flags (--gpu-sketch, --strand-preserved,
--min-kmer-count, --exact-count: accepted, unused by --create-db upstream too), a path from the sketches without the
matrices, and more than one GPU.

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


def write_lineage_csv(outfile, names, clustering, suffix='_Lineage', queryNames=None):
    """writeClusterCsv(outfile, names, names, clustering, 'phandango', None, queryNames, suffix) (PopPUNK/plot.py:
    598-760): `id` and one `<type><suffix>` column per clustering, one row per name, as pandas' to_csv writes them; with
    queryNames also `Status` (Query / Reference) and `Status:colour`."""
    first = next(iter(clustering))
    queries = None if queryNames is None else set(queryNames)
    rows = []
    for name, label in zip(names, isolateNameToLabel(names)):
        if name not in clustering[first]:
            sys.stderr.write("Cannot find " + name + " in clustering\n")
            sys.exit(1)
        rows.append([label] + [clustering[cluster_type][name] for cluster_type in clustering])
        if queries is not None:
            rows[-1] += ["Query", "#ff0000"] if name in queries else ["Reference", "#000000"]
    sys.stderr.write("Parsed data, now writing to CSV\n")
    with open(outfile, 'w', newline='') as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(['id'] + [cluster_type + suffix for cluster_type in clustering]
                     + ([] if queries is None else ['Status', 'Status:colour']))
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
    return _device_ranks(oi, oj, od, seg_off, depth, ranks, reciprocal_only, count_unique_distances, epsilon)


def _device_ranks(oi, oj, od, seg_off, depth, ranks, reciprocal_only, count_unique_distances, epsilon):
    """The rank call and the cluster sweep over sorted lists in strain_knn_dev's layout (its own or
    strain_extend_dev's), and the split of everything by strain: what _device_fit and _device_extend return."""
    torch = engine._torch()
    dev = oi.device
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


def _device_extend(members, seg_off, queries, qry_off, stored, qr, qq, n_ref, n_qry, depth, col, ranks,
                   reciprocal_only, count_unique_distances, epsilon, device_id=0):
    """The three device calls of extend_strain_lineages -> what _device_fit returns, over the extended strains (members,
    then queries).  stored: the (j, dist) lists of all strains back to back in strain_knn_dev's layout; qr, qq: CUDA
    tensors are read where they are, numpy arrays uploaded to device_id.  The host tests replace this function with the
    numpy model."""
    torch = engine._torch()

    def resident(a):
        if a is None or getattr(a, "is_cuda", False):
            return a
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:%d" % device_id)
    qr, qq = resident(qr), resident(qq)
    dev = qr.device
    as_t = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)
    oi, oj, od = engine.strain_extend_dev(as_t(members, np.int64), seg_off, as_t(queries, np.int64), qry_off,
                                          as_t(stored[0], np.int64), as_t(stored[1], np.float32), qr, qq, n_ref, n_qry,
                                          depth, col, models.EPSILON)
    return _device_ranks(oi, oj, od, np.asarray(seg_off) + np.asarray(qry_off), depth, ranks, reciprocal_only,
                         count_unique_distances, epsilon)


def _stored_rows(model, n_s):
    """A loaded model's nn_dists as (j, dist) in strain_knn_dev's layout -- min(depth, n_s - 1) entries a row, rows in
    order, each non-decreasing in distance (a stable sort per row puts a matrix that is not in that order into it) -- or
    None when a row has another length."""
    coo = model.nn_dists.tocoo()
    if coo.shape != (n_s, n_s):
        raise RuntimeError("a lineage model of %d samples for a strain of %d members" % (coo.shape[0], n_s))
    d_s = min(model.max_search_depth, n_s - 1)
    if len(coo.row) != n_s * d_s or not np.array_equal(np.bincount(coo.row, minlength=n_s), np.full(n_s, d_s)):
        return None
    order = np.lexsort((coo.data, coo.row))              # (stable: entries of equal distance keep their order)
    return coo.col[order].astype(np.int64), coo.data[order].astype(np.float32)


def extend_strain_lineages(fitted, names_of, qNames, strain_of_query, qr, qq, rNames, device_id=0):
    """The lineage branch of assign_query_hdf5 (PopPUNK/assign.py:528-573) for every strain that received queries, in
    one pass over the two resident matrices.
    fitted: {strain: a fitted or loaded models.LineageRanks}; names_of: {strain: its member names in the model's row
    order}; rNames / qNames: the names the matrices are indexed by; strain_of_query: {query name: strain}, or a
    sequence along qNames (None: no strain); qr: float32 [len(qNames) * len(rNames), 2], row q * n_ref + r; qq: float32
    long form of the queries (may be None when no strain has two).  CUDA tensors are read where they are, numpy arrays
    uploaded to device_id.
    Queries whose strain has no model in `fitted` are left out; strains without queries are not touched.  Returns
    {strain: (model, lineage_clusters, overall_lineage)} in fitted's order, as fit_strain_lineages does: a NEW model whose
    nn_dists and lower_rank_dists are array for array what LineageRanks.extend leaves on that strain alone,
    {rank: {name: number}} over members then queries in printClusters' order (fresh numbers by size), and
    createOverallLineage's dict.
    All models must share ranks, search depth, flags, resolution and distance column (RuntimeError otherwise).  A model
    whose rows are not sorted by distance is put in order on the host (a stable sort per row); a model with a row of
    another length than min(depth, n_s - 1) -- which no fit or extend of this package or the reference writes --
    goes through LineageRanks.extend on its own, with the same results."""
    if not hasattr(strain_of_query, "get"):
        strain_of_query = dict(zip(qNames, strain_of_query))
    placed = defaultdict(list)
    for q, name in enumerate(qNames):
        strain = strain_of_query.get(name)
        if strain is not None and strain in fitted:
            placed[strain].append(q)
    todo = [strain for strain in fitted if strain in placed]
    if not todo:
        return {}
    proto = fitted[todo[0]]
    scheme = lambda m: (m.ranks, m.max_search_depth, m.reciprocal_only, m.count_unique_distances, m.resolution, m.dist_col)
    for strain in todo:
        if not fitted[strain].fitted:
            raise RuntimeError("Trying to extend an unfitted model")
        if scheme(fitted[strain]) != scheme(proto):
            raise RuntimeError("the lineage models of strains %s and %s differ in ranks, search depth or flags"
                               % (todo[0], strain))
    n_ref, n_qry = len(rNames), len(qNames)
    if int(qr.shape[0]) != n_qry * n_ref:
        raise RuntimeError("the query x reference matrix does not hold the %d pairs of %d queries and %d references"
                           % (n_qry * n_ref, n_qry, n_ref))
    if qq is not None and int(qq.shape[0]) != n_qry * (n_qry - 1) // 2:
        raise RuntimeError("the query matrix does not hold the %d pairs of %d queries" % (n_qry * (n_qry - 1) // 2, n_qry))
    index = {name: k for k, name in enumerate(rNames)}
    rank_list, depth = proto.ranks, proto.max_search_depth

    def new_model():
        return models.LineageRanks(rank_list, depth, proto.reciprocal_only, proto.count_unique_distances,
                                   proto.resolution, dist_col=proto.dist_col, threads=proto.threads)

    def clusters_of(numbers_by_rank, isolates):
        lineage_clusters = {}
        for rank, mine in zip(rank_list, numbers_by_rank):
            order = np.argsort(mine, kind="stable")
            lineage_clusters[rank] = {isolates[k]: int(mine[k]) for k in order}
        return lineage_clusters

    batch, rows_of, alone = [], {}, []
    for strain in todo:
        rows_of[strain] = _stored_rows(fitted[strain], len(names_of[strain]))
        (batch if rows_of[strain] is not None else alone).append(strain)
    out = {}
    if batch:
        members = np.asarray([index[name] for strain in batch for name in names_of[strain]], dtype=np.int64)
        queries = np.asarray([q for strain in batch for q in placed[strain]], dtype=np.int64)
        seg_off = np.concatenate([[0], np.cumsum([len(names_of[strain]) for strain in batch])]).astype(np.int64)
        qry_off = np.concatenate([[0], np.cumsum([len(placed[strain]) for strain in batch])]).astype(np.int64)
        stored = tuple(np.concatenate([rows_of[strain][k] for strain in batch]) for k in (0, 1))
        lists, outputs, numbers = _device_extend(members, seg_off, queries, qry_off, stored, qr, qq, n_ref, n_qry, depth,
                                                 proto.dist_col, rank_list, proto.reciprocal_only,
                                                 proto.count_unique_distances, proto.resolution, device_id)
        ext_off = seg_off + qry_off
        for s, strain in enumerate(batch):
            n_x = int(ext_off[s + 1] - ext_off[s])
            model = new_model()
            li, lj, ld = lists[s]
            model.nn_dists = model._coo(ld, li, lj, n_x)
            for q, rank in enumerate(rank_list):
                ri, rj, rd = outputs[s][q]
                model.lower_rank_dists[rank] = model._coo(rd, ri, rj, n_x)
            model.fitted = True
            isolates = list(names_of[strain]) + [qNames[q] for q in placed[strain]]
            out[strain] = (model, clusters_of(numbers[:, ext_off[s]:ext_off[s + 1]], isolates))
    for strain in alone:
        out[strain] = _extend_alone(fitted[strain], new_model(), [index[name] for name in names_of[strain]],
                                    placed[strain], qr, qq, n_ref, n_qry)
        isolates = list(names_of[strain]) + [qNames[q] for q in placed[strain]]
        out[strain] = (out[strain][0], clusters_of(out[strain][1], isolates))
    return {strain: out[strain] + (createOverallLineage(rank_list, out[strain][1]),) for strain in todo}


def _extend_alone(old, model, members, queries, qr, qq, n_ref, n_qry):
    """One strain through the calls that take a strain at a time, as LineageRanks.extend makes them (its long form of
    the queries cannot state a single query; the square can) -> (model, numbers per rank)."""
    from . import poppunk_refine
    from .network import cluster_numbers
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    mem, qry = np.asarray(members, dtype=np.int64), np.asarray(queries, dtype=np.int64)
    col, floor = model.dist_col, np.float32(models.EPSILON)
    rect = host(qr)[qry[None, :] * np.int64(n_ref) + mem[:, None], col].astype(np.float32)
    square = np.zeros((len(qry), len(qry)), dtype=np.float32)
    a, b = np.triu_indices(len(qry), 1)
    if len(a):
        lo, hi = np.minimum(qry[a], qry[b]), np.maximum(qry[a], qry[b])
        square[a, b] = square[b, a] = host(qq)[lo * (2 * n_qry - lo - 1) // 2 + (hi - lo - 1), col]
    rect, square = np.where(rect < floor, floor, rect), np.where(square < floor, floor, square)
    n_x = len(mem) + len(qry)
    coo = old.nn_dists.tocoo()
    higher = poppunk_refine.extend_arrays((coo.row, coo.col, coo.data), square, rect, model.max_search_depth,
                                          model.threads)
    model.nn_dists = model._coo(higher[2], higher[0], higher[1], n_x)
    model._ranks_from(higher, n_x)
    model.fitted = True
    numbers = []
    for rank in model.ranks:
        coo = model.lower_rank_dists[rank]
        numbers.append(cluster_numbers((np.stack([coo.row, coo.col], axis=1), n_x)))
    return model, numbers


def get_options(argv=None):
    parser = argparse.ArgumentParser(description="Lineages within the strains of a database, fitted on the device",
                                     prog="python -m poppunk_amd.lineages")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument('--create-db', type=str, default=None, help="strain database to fit lineages within")
    mode.add_argument('--query-db', type=str, default=None,
                      help="sketched query database to assign to strains and to the lineages within them")
    parser.add_argument('--db-scheme', required=True,
                        help="pickle describing the lineage databases (--create-db writes it, --query-db reads it)")
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


def _query_distances(ref_db, query_db, rNames, qNames, kmers, threads=1, deviceid=0):
    """(query x reference float32 [n_qry * n_ref, 2], query x query long form) from the two sketched databases.  The
    tests put recorded matrices in this function's place."""
    from . import sketchlib
    qr = sketchlib.queryDatabase(rNames, qNames, ref_db, query_db, kmers, self=False, threads=threads, deviceid=deviceid)
    qq = (sketchlib.queryDatabase(qNames, qNames, query_db, query_db, kmers, self=True, threads=threads,
                                  deviceid=deviceid) if len(qNames) > 1 else np.zeros((0, 2), dtype=np.float32))
    return qr, qq


def _load_strain_model(model_dir):
    path = os.path.join(model_dir, os.path.basename(model_dir) + '_fit.npz')
    for cls in (models.RefineBoundary, models.BGMMModel, models.DBSCANModel):
        try:
            return cls.from_npz(path)
        except ValueError:
            continue
    raise RuntimeError("no refine, BGMM or DBSCAN fit in " + path)


def _assign_strains(rNames, qNames, qr, qq, model_dir, external_clustering, output, core, accessory, kmers):
    """assign_query_hdf5 for the strains (PopPUNK/lineages.py:390-414) on loaded pieces -> isolateClustering: the strain
    network by its components, read from <model_dir>_clusters.csv, and assign.assign_query_clusters in joint mode.  The
    tests put a recorded placing in this function's place."""
    from . import assign
    from .utils import readIsolateTypeFromCsv
    old_cluster_file = os.path.join(model_dir, os.path.basename(model_dir) + '_clusters.csv')
    cluster_of = readIsolateTypeFromCsv(old_cluster_file, mode='clusters', return_dict=True)['Cluster']
    numbers = {}
    labels = np.asarray([numbers.setdefault(cluster_of[name], len(numbers)) for name in rNames], dtype=np.int32)
    refnet = assign.ReferenceNetwork((np.zeros((0, 2), dtype=np.int64), len(rNames)), rNames, old_cluster_file,
                                     labels=labels)
    fit_type = 'core_refined' if core else 'accessory_refined' if accessory else 'default'
    dbFuncs = {'queryDatabase': lambda **kw: qq}             # (computed once for all queries)
    return assign.assign_query_clusters(dbFuncs, refnet, qNames, qr, _load_strain_model(model_dir), output,
                                        kmers=kmers, fit_type=fit_type,
                                        external_clustering=external_clustering)["isolateClustering"]


def query_db(args):
    """PopPUNK/lineages.py:329-466 on loaded pieces; see the module docstring for what differs."""
    from .sketchdb import getSeqsInDb
    with open(args.db_scheme, 'rb') as pickle_file:
        ref_db, rlist, model_dir, clustering_file, args.clustering_col_name, distances, \
            kmers, sketch_sizes, codon_phased, max_search_depth, rank_list, use_accessory, min_count, \
            count_unique_distances, reciprocal_only, strand_preserved, core, accessory, lineage_dbs = \
            pickle.load(pickle_file)

    previous_clustering_file = os.path.join(model_dir, os.path.basename(model_dir) + '_clusters.csv')
    external_clustering = None
    if clustering_file != previous_clustering_file:
        external_clustering = clustering_file
    if args.output is None:
        sys.stderr.write("Need an output file name\n")
        sys.exit(1)
    if ref_db == args.output:
        sys.stderr.write("--output and --ref-db must be different to "
                         "prevent overwrite.\n")
        sys.exit(1)
    if not os.path.isdir(args.output):
        os.makedirs(args.output)

    rNames = distfile.readPickle(distances, enforce_self=True, distances=False)[0]
    query_stem = os.path.join(args.query_db, os.path.basename(args.query_db))
    qNames = list(getSeqsInDb(query_stem + ('.h5' if os.path.exists(query_stem + '.h5') else '.npz')))
    qr, qq = _query_distances(ref_db, args.query_db, rNames, qNames, kmers, args.threads, args.deviceid)
    isolateClustering = _assign_strains(rNames, qNames, qr, qq, model_dir, external_clustering, args.output, core,
                                        accessory, kmers)

    clustering_type = 'core' if core else 'combined'
    if accessory:
        clustering_type = 'accessory'
    if clustering_type not in isolateClustering:             # (assign_query_clusters names its one clustering 'combined')
        clustering_type = 'combined'
    in_query = set(qNames)
    query_strains = {}
    for isolate, strain in isolateClustering[clustering_type].items():
        if isolate in in_query:
            query_strains.setdefault(strain, []).append(isolate)

    # every strain's lineage model and names, then one pass for all of them
    fitted, names_of, strain_of_query = {}, {}, {}
    for strain in query_strains:
        if strain in lineage_dbs.keys():
            prefix = lineage_dbs[strain]
            fitted[strain] = models.LineageRanks.load(prefix)
            names_of[strain] = distfile.readPickle(os.path.join(prefix, os.path.basename(prefix) + '.dists'),
                                                   enforce_self=True, distances=False)[0]
            for isolate in query_strains[strain]:
                strain_of_query[isolate] = strain
    extended = extend_strain_lineages(fitted, names_of, qNames, strain_of_query, qr, qq, rNames, args.deviceid)
    overall_lineage = {}
    for strain in fitted:
        _, _, overall_lineage[strain] = extended[strain]
        placed = [name for name in qNames if strain_of_query.get(name) == strain]
        # (the reference writes this one path once per strain: the last strain's file remains)
        write_lineage_csv(os.path.join(args.output, os.path.basename(args.output) + '_lineages.csv'),
                          list(names_of[strain]) + placed, overall_lineage[strain], queryNames=placed)
    if not overall_lineage:
        raise RuntimeError("no strain with a lineage database received a query: there is no clustering to write "
                           "(the reference fails here on an empty dict)")
    print_overall_clustering(overall_lineage, args.output + '.csv', qNames)


def main(argv=None):
    args = get_options(argv)
    if args.create_db is not None:
        create_db(args)
    else:
        query_db(args)


if __name__ == '__main__':
    main()
    sys.exit(0)
