"""Cluster QC over the boundaries of --multi-boundary: scripts/poppunk_iterate.py on the MI355X.

    read_next_cluster_file(db_prefix), is_nested(cluster_dict, child_members, node_list)      the script's two functions
    iterate_clusters(levels | db_prefix, names, dist, cutoff=0.1, output=None)
        -> {"family", "sorted", "avg_pi", "parents", "cut_clusters", "cut_assignment", "newick"}

The script nests the clusterings of all boundaries into one family (:156-182), gives every cluster of the family its
mean core distance (:184-215), hangs the family on a tree (:217-241) and cuts that tree where the mean, as a
proportion of the largest one, crosses `cutoff` (:250-304).

Avg_Pi.  Upstream runs one pp_sketchlib.queryDatabase per cluster, so a pair is recomputed at every level that holds
it.  Here the core column of the resident matrix is read ONCE (engine.cluster_pair_sums_dev): every pair goes to the
bucket of the first boundary at which its two samples share a cluster, and `cluster_totals` adds the buckets of a
cluster's sub-clusters on the host.  The sums are fixed point (2^-shift units), so they are the same bits on every run
and a mean is within 2^-(shift + 1) of the float64 mean of the float32 values.  The reference's value is numpy's
float32 np.mean over the same values: agreement is to float32 summation error, not to the bit.

The tree cut needs treeswift upstream, which is not installed here: it is restated by reading and UNPINNED.  Two
things are kept as the script has them: its test for "an ancestor is also selected" looks a label up in a set of
nodes, which never matches, so no ancestor is ever dropped; and an edge length equal to the cutoff is neither below
nor above it.  Where the script iterates a Python set (members of a cluster, the selected nodes, the leftover
singletons) the order here is that of `names`, and of selection.
"""
import os
from collections import defaultdict

import numpy as np


def read_next_cluster_file(db_prefix):
    """The generator of scripts/poppunk_iterate.py:78-112: for k = 0, 1, ... while `<db_prefix>_boundary<k>_clusters.csv`
    exists, (every cluster {id: set of names} in the file's order, those of more than one name, k)."""
    import csv
    import itertools
    for k in itertools.count():
        path = "%s_boundary%d_clusters.csv" % (db_prefix, k)
        if not os.path.isfile(path):
            return
        with open(path, newline="") as f:
            rows = list(csv.reader(f))[1:]
        everything = defaultdict(set)
        for name, cluster in rows:
            everything[int(cluster)].add(name)
        several = defaultdict(set, {c: m for c, m in everything.items() if len(m) > 1})
        yield everything, several, k


def is_nested(cluster_dict, child_members, node_list):
    """scripts/poppunk_iterate.py:115-136: of the clusters named in node_list that hold every member of
    child_members, the smallest (the first of equal sizes); None when there is none."""
    holders = [node for node in node_list if cluster_dict[node] >= child_members]
    return min(holders, key=lambda node: len(cluster_dict[node])) if holders else None


def check_nested(levels):
    """ValueError unless two samples that share a cluster at level t share one at every later level (the precondition
    of ppk_cluster_pair_sums_dev): every cluster of level t must lie in ONE cluster of level t + 1."""
    levels = np.asarray(levels)
    if levels.ndim != 2:
        raise ValueError("levels must be [n_levels, n]")
    for t in range(levels.shape[0] - 1):
        pairs = np.unique(np.stack([levels[t], levels[t + 1]]), axis=1).shape[1]
        if pairs != np.unique(levels[t]).size:
            raise ValueError("levels are not nested: a cluster of level %d is split at level %d" % (t, t + 1))


def levels_of_files(db_prefix, names):
    """The boundary files as a level matrix: int32 [n_files, n], row k = every name's cluster id in file k."""
    index = {name: v for v, name in enumerate(names)}
    rows = []
    for all_clusters, _, _ in read_next_cluster_file(db_prefix):
        row = np.zeros(len(names), dtype=np.int32)
        seen = 0
        for cluster, members in all_clusters.items():
            for name in members:
                row[index[name]] = cluster
                seen += 1
        if seen != len(names):
            raise ValueError("a boundary file does not list every sample once")
        rows.append(row)
    if not rows:
        raise ValueError("no boundary files at " + db_prefix)
    return np.stack(rows)


def family_of_levels(levels, names):
    """The script's family (:156-182) from a NESTED level matrix (check_nested) -> (family {id: set of names}, where
    {id: (level, cluster number)}, the ids by size descending (stable), the set of all names).

    The script admits the first file's clusters of two or more names under their own ids, then every later cluster
    that is new and is inside, around or apart from each one admitted so far, numbering on from the largest id; it
    meets a file's clusters in the file's order, which printClusters makes size descending, then id.  Over nested
    levels a cluster can only be inside, around or apart from an earlier one, so the test that decides is "new": a
    cluster of level t is one already met exactly when the cluster of level t - 1 around its first vertex has the
    same size.  That makes the family n_levels * n work instead of a set comparison per pair of clusters."""
    levels = np.asarray(levels)
    names = list(names)
    check_nested(levels)
    family, where = {}, {}
    next_id = None
    size_before = None                   # per vertex: the size of its cluster one level down
    for t, row in enumerate(levels):
        ids, first, inverse, sizes = np.unique(row, return_index=True, return_inverse=True, return_counts=True)
        for k in np.lexsort((ids, -sizes)).tolist():
            if sizes[k] < 2:
                break                    # (sorted by size: only singletons follow)
            if t > 0 and size_before[first[k]] == sizes[k]:
                continue
            if t == 0:
                cluster = int(ids[k])
            else:
                next_id += 1
                cluster = next_id
            family[cluster] = {names[v] for v in np.flatnonzero(row == ids[k]).tolist()}
            where[cluster] = (t, int(ids[k]))
        if t == 0:
            next_id = max(family)        # ValueError when the first level is all singletons, as upstream's max()
        size_before = sizes[inverse.reshape(-1)]
    by_size = sorted(family, key=lambda c: -len(family[c]))
    return family, where, by_size, set(names)


def dense_levels(levels):
    """Every level renumbered 1 .. K_t in the order of its ids (the device wants numbers in [1, n])."""
    levels = np.asarray(levels)
    out = np.empty(levels.shape, dtype=np.int32)
    for t in range(levels.shape[0]):
        out[t] = np.unique(levels[t], return_inverse=True)[1].reshape(-1) + 1
    return out


def cluster_totals(levels, bucket_sum, bucket_cnt):
    """From the buckets of ppk_cluster_pair_sums (int64 [n_levels, n + 1]: the pairs that FIRST meet at (t, c)) to the
    totals over all pairs of every cluster: total[t][c] = bucket[t][c] + the totals of the clusters of level t - 1
    inside it.  levels: int [n_levels, n], nested, numbers in [1, n].  n_levels * n work.  -> (sum, cnt) int64."""
    levels = np.asarray(levels, dtype=np.int64)
    tot_s = np.array(bucket_sum, dtype=np.int64, copy=True)
    tot_c = np.array(bucket_cnt, dtype=np.int64, copy=True)
    for t in range(1, levels.shape[0]):
        # one representative vertex per cluster of level t - 1 names the cluster of level t that holds it
        prev, rep = np.unique(levels[t - 1], return_index=True)
        np.add.at(tot_s[t], levels[t][rep], tot_s[t - 1][prev])
        np.add.at(tot_c[t], levels[t][rep], tot_c[t - 1][prev])
    return tot_s, tot_c


def cluster_means(levels, bucket_sum, bucket_cnt, shift):
    """float64 [n_levels, n + 1]: the mean over the pairs of every cluster (NaN: no pairs).  Each is the quotient of two
    exact integers, total / (count * 2^shift), rounded once (Python's int / int)."""
    tot_s, tot_c = cluster_totals(levels, bucket_sum, bucket_cnt)
    means = np.full(tot_s.shape, np.nan)
    for t, c in zip(*np.nonzero(tot_c)):
        means[t, c] = int(tot_s[t, c]) / (int(tot_c[t, c]) << int(shift))
    return means


def nest_family(iterated_clusters, sorted_clusters, all_samples):
    """The script's tree (:217-241) -> (parents {id: the id it hangs under, 'root', or None}, leftover {id or 'root':
    the samples hanging directly under it}).  Largest first, every cluster goes under the smallest node placed so far
    whose REMAINING samples hold all of its own, and takes them away from that node."""
    remaining = {"root": set(all_samples)}
    remaining.update((c, set(members)) for c, members in iterated_clusters.items())
    placed, parents = ["root"], {}
    for c in sorted_clusters:
        above = is_nested(remaining, remaining[c], placed)
        parents[c] = above
        if above is not None:
            remaining[above] -= remaining[c]
        placed.append(c)
    return parents, remaining


def cut_tree(parents, leftover, pi_values, cutoff, names):
    """The script's cut (:250-289), UNPINNED (see the module docstring) -> the selected cluster ids, in the order they
    are first selected.  Edge lengths are pi / max(pi)."""
    max_pi = max([-1.0] + [pi_values[c] for c in pi_values])
    length = {c: pi_values[c] * (1 / max_pi) for c in parents}

    def attached(c):                                  # reachable from the root
        while c is not None and c != "root":
            c = parents.get(c)
        return c == "root"

    order = {name: k for k, name in enumerate(names)}
    cut = []
    for holder in ["root"] + [c for c in parents]:
        if holder != "root" and not attached(holder):
            continue
        for _leaf in sorted(leftover[holder], key=order.get):
            parent_node = holder
            if parent_node == "root":
                continue
            if length[parent_node] < cutoff and parents[parent_node] == "root":
                if parent_node not in cut:
                    cut.append(parent_node)
            elif length[parent_node] < cutoff:
                while length[parent_node] < cutoff:
                    child_node = parent_node
                    parent_node = parents[child_node]
                    if parent_node == "root":
                        if child_node not in cut:
                            cut.append(child_node)
                        break
                    if length[child_node] < cutoff and length[parent_node] > cutoff:
                        if child_node not in cut:
                            cut.append(child_node)
                        break
    return cut


def family_newick(parents, leftover, sorted_clusters, names):
    """The family as a Newick string through trees.newick: inner nodes 'root' and 'cluster<id>', leaves the samples
    (treeswift writes no lengths for this tree; trees.newick writes 0.00000)."""
    from . import trees
    names = list(names)
    index = {name: v for v, name in enumerate(names)}
    t = trees.Tree(len(names))
    children = defaultdict(list)
    for c in sorted_clusters:
        if parents[c]:
            children[parents[c]].append(c)
    node = {}
    # children before parents: the reverse of a preorder from the root
    stack, preorder = ["root"], []
    while stack:
        c = stack.pop()
        preorder.append(c)
        stack.extend(children[c])
    for c in reversed(preorder):
        kids = [node[k] for k in children[c]] + [index[s] for s in sorted(leftover[c], key=index.get)]
        node[c] = t.add_node(kids, "root" if c == "root" else "cluster" + str(c))
    t.root = node["root"]
    return trees.newick(t, names)


def iterate_clusters(levels, names, dist, cutoff=0.1, output=None, device_id=0):
    """scripts/poppunk_iterate.py from its first cluster file to its last line.

    levels: an int [n_levels, n] matrix of cluster ids (multi_refine's first return value), or the prefix
    `<db>/<basename>` of the `_boundary<k>_clusters.csv` files.  names: the n sample names in vertex order.  dist: the
    float32 [n(n-1)/2, 2] distance matrix (unscaled), numpy or a resident CUDA tensor; column 0 is read.
    Returns a dict: family {id: set of names}, sorted (ids, size descending), avg_pi {id: mean core distance},
    parents {id: parent id, 'root' or None}, cut_clusters (ids), cut_assignment {name: number}, newick.
    With `output`, writes `<output>.clusters.csv` (Cluster,Avg_Pi,Taxa), `<output>.tree.nwk` and
    `<output>.cutoff_clusters.csv` (Isolate,Cluster)."""
    if cutoff >= 1 or cutoff <= 0:
        raise RuntimeError("--cutoff must be between 0 and 1\n")
    import torch
    from . import engine
    names = list(names)
    if isinstance(levels, (str, bytes)) or hasattr(levels, "__fspath__"):
        levels = levels_of_files(os.fspath(levels), names)
    levels = np.asarray(levels)
    if levels.ndim != 2 or levels.shape[1] != len(names):
        raise ValueError("levels must be [n_levels, %d]" % len(names))
    check_nested(levels)
    family, where, sorted_clusters, all_samples = family_of_levels(levels, names)

    dense = dense_levels(levels)
    if isinstance(dist, torch.Tensor):
        dist_t = dist
    else:
        dist_t = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32)).to("cuda:%d" % device_id)
    levels_t = torch.from_numpy(dense).to(dist_t.device)
    s, c, shift = engine.cluster_pair_sums_dev(dist_t, levels_t, col=0)
    means = cluster_means(dense, s.cpu().numpy(), c.cpu().numpy(), shift)
    index = {name: v for v, name in enumerate(names)}
    pi_values = {}
    for cluster in sorted_clusters:
        t, _ = where[cluster]
        v = index[next(iter(family[cluster]))]
        pi_values[cluster] = float(means[t, dense[t, v]])

    parents, leftover = nest_family(family, sorted_clusters, all_samples)
    newick = family_newick(parents, leftover, sorted_clusters, names)
    cut = cut_tree(parents, leftover, pi_values, cutoff, names)
    assignment = {}
    lines = []
    # (a sample of two selected clusters, one inside the other, is listed under both, as upstream; the dict keeps the
    # later one)
    for idx, cluster in enumerate(cut):
        for sample in sorted(family[cluster], key=index.get):
            assignment[sample] = idx + 1
            lines.append("%s,%d\n" % (sample, idx + 1))
    singletons = [name for name in names if name not in assignment]
    for idx, sample in enumerate(singletons):
        assignment[sample] = idx + len(cut) + 1
        lines.append("%s,%d\n" % (sample, idx + len(cut) + 1))

    if output is not None:
        with open(f"{output}.tree.nwk", "w") as f:
            f.write(newick)
        with open(f"{output}.clusters.csv", "w") as f:
            f.write("Cluster,Avg_Pi,Taxa\n")
            for cluster in sorted_clusters:
                taxa = ';'.join(sorted(family[cluster], key=index.get))
                f.write(f"{str(cluster)},{str(pi_values[cluster])},{taxa}\n")
        with open(f"{output}.cutoff_clusters.csv", "w") as f:
            f.write("Isolate,Cluster\n")
            f.writelines(lines)
    return {"family": family, "sorted": sorted_clusters, "avg_pi": pi_values, "parents": parents,
            "cut_clusters": cut, "cut_assignment": assignment, "newick": newick}
