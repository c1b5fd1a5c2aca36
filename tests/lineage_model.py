"""ppk_strain_knn_dev / ppk_strain_ranks_dev (include/ppk.h "Lineages within every strain") restated in
numpy, strain by strain, through the steps a caller takes today: prune the long form to the strain, oracle.long_to_square,
oracle.knn, oracle.lower_rank per rank; then connected components and printClusters' numbering as include/ppk.h states
it for ppk_cluster_sweep_dev.  (oracle.knn and oracle.lower_rank are restatements by reading: parity with the
reference's C++ is unpinned, see oracle/oracle.py.)"""
import numpy as np

from oracle import oracle


def strain_square(dist, n, members, col):
    """The strain's square matrix in LOCAL order: the pruned long form is in ascending-id order, so it is permuted."""
    members = np.asarray(members, dtype=np.int64)
    keep = np.sort(members)
    sq = oracle.long_to_square(oracle.prune_long(np.asarray(dist, dtype=np.float32), n, keep)[:, col])
    at = np.searchsorted(keep, members)
    return np.ascontiguousarray(sq[np.ix_(at, at)])


def strain_knn(dist, n, members, seg_off, depth, col=0):
    """(i, j, dist) with local indices, strain by strain; -0.0 comes back as 0.0 (the device's keys fold it)."""
    oi, oj, od = [], [], []
    for s in range(len(seg_off) - 1):
        mem = members[seg_off[s]:seg_off[s + 1]]
        i, j, d = oracle.knn(strain_square(dist, n, mem, col), min(depth, len(mem) - 1))
        oi.append(i)
        oj.append(j)
        od.append(d + np.float32(0.0))
    return np.concatenate(oi), np.concatenate(oj), np.concatenate(od).astype(np.float32)


def components(n, edges):
    """Labels 0 .. K - 1 in the order of each component's smallest vertex."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.asarray([find(v) for v in range(n)])
    _, labels = np.unique(roots, return_inverse=True)       # a root is its component's smallest vertex
    return labels


def print_clusters_numbers(labels):
    """1-based numbers: by size descending, equal sizes by component index DESCENDING (len - rankdata(sizes,
    'ordinal'), PopPUNK/network.py:1538-1545 as include/ppk.h reads it)."""
    sizes = np.bincount(labels)
    order = np.argsort(sizes, kind="stable")                # ordinal ranks 1 .. K: ties by index ascending
    rank = np.empty(len(sizes), dtype=np.int64)
    rank[order] = np.arange(1, len(sizes) + 1)
    return (len(sizes) - rank + 1)[labels].astype(np.int32)


def strain_ranks(knn_lists, seg_off, depth, ranks, reciprocal_only=False, count_unique_distances=False,
                 epsilon=1e-10):
    """From strain_knn's lists: prefix int32 [R, m]; the level stream as a sorted int64 [k, 3] array of (position of
    the lower member, position of the higher, level); per-strain cluster numbers int32 [R, m]; and per strain and
    rank lowerRank's own (i, j, dist) output (what LineageRanks stores)."""
    oi, oj, od = knn_lists
    m, n_ranks = int(seg_off[-1]), len(ranks)
    prefix = np.zeros((n_ranks, m), dtype=np.int32)
    numbers = np.zeros((n_ranks, m), dtype=np.int32)
    stream, outputs = [], []
    at = 0
    for s in range(len(seg_off) - 1):
        seg0, n_s = int(seg_off[s]), int(seg_off[s + 1] - seg_off[s])
        cnt = n_s * min(depth, n_s - 1)
        li, lj, ld = oi[at:at + cnt], oj[at:at + cnt], od[at:at + cnt]
        at += cnt
        level_of, per_rank = {}, []
        for q, rank in enumerate(ranks):
            ki, kj, _ = oracle.lower_rank(li, lj, ld, n_s, rank, False, count_unique_distances, epsilon)
            prefix[q, seg0:seg0 + n_s] = np.bincount(ki, minlength=n_s)
            out = (oracle.lower_rank(li, lj, ld, n_s, rank, True, count_unique_distances, epsilon)
                   if reciprocal_only else (ki, kj, _))
            per_rank.append(out)
            for a, b in zip(out[0].tolist(), out[1].tolist()):
                level_of.setdefault((min(a, b), max(a, b)), q)
            numbers[q, seg0:seg0 + n_s] = print_clusters_numbers(components(n_s, zip(out[0], out[1])))
        stream += [(seg0 + a, seg0 + b, q) for (a, b), q in level_of.items()]
        outputs.append(per_rank)
    stream = np.asarray(sorted(stream), dtype=np.int64).reshape(-1, 3)
    return prefix, stream, numbers, outputs
