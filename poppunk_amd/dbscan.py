"""The host half of the HDBSCAN model (`--fit-model dbscan`): the hierarchy over a device-built minimum spanning tree.

The device gives the squared core distances and the minimum spanning tree of the mutual-reachability graph, sorted
under the total order (mr2, min(a, b), max(a, b)) (include/ppk.h, "DBSCAN").  What follows is
sequential, O(n log n) on at most 100 000 points, and stays here, in numpy and plain Python:

  * `single_linkage(a, b, mr2, n)` : union-find over the sorted edges -> the single-linkage tree
  * `condense(tree, n, c)`         : the condensed tree for min_cluster_size c
  * `select_eom(ct)`               : stabilities and excess-of-mass selection (allow_single_cluster=False,
                                     cluster_selection_epsilon=0, no max_cluster_size)
  * `labels(ct, selected)`         : -1 noise, clusters numbered by their smallest member index
  * `fit_tree(a, b, mr2, n, c)`    : the four in a row -> `Tree`, the state the assignment reads

These restate the rules of sklearn/cluster/_hdbscan/_tree.pyx (_condense_tree, _compute_stability, _get_clusters,
_do_labelling) with lambda = 1 / d and lambda = +inf at d = 0.  Clusters are numbered from the root (0) in the order
they are born when the single-linkage nodes are visited from the last merge to the first, the side holding the
edge's lower end first.

`findWithinLabel`, `findBetweenLabel`, `evaluate_dbscan_clusters` and the parameter rules are PopPUNK's glue
(PopPUNK/dbscan.py:69-123, PopPUNK/bgmm.py:71-97, PopPUNK/models.py:490-610).  scipy and sklearn are not needed.
"""
import numpy as np


# ---- PopPUNK's parameter rules (models.py:515-518) ------------------------------------------------------------
def min_samples_for(n, min_cluster_prop):
    return min(max(int(min_cluster_prop * n), 10), 1023)


def min_cluster_size_for(n):
    return max(int(0.01 * n), 10)


def next_parameters(min_samples, min_cluster_size):
    """The step at the end of the fitting loop's body (models.py:589-592)."""
    if min_cluster_size < min_samples / 2:
        min_samples = min_samples // 10
    return min_samples, int(min_cluster_size / 2)


def loop_continues(indistinct, min_samples, min_cluster_size):
    """The fitting loop's condition (models.py:541)."""
    return bool(indistinct) and min_cluster_size >= min_samples and min_samples >= 10


def acceptable(n_clusters, max_num_clusters):
    """models.py:551: only such a fit is looked at for distinct clusters."""
    return 1 < n_clusters <= max_num_clusters


# ---- hierarchy ---------------------------------------------------------------------------------------------------
def single_linkage(a, b, mr2, n):
    """(left, right, dist, size), one entry per edge: node n + k is the merge of edge k.  `left` holds a[k]."""
    a = np.asarray(a, dtype=np.int64).tolist()
    b = np.asarray(b, dtype=np.int64).tolist()
    if len(a) != n - 1:
        raise ValueError("a spanning tree of %d points has %d edges" % (n, n - 1))
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    left = np.empty(n - 1, dtype=np.int64)
    right = np.empty(n - 1, dtype=np.int64)
    sz = np.empty(n - 1, dtype=np.int64)
    for k in range(n - 1):
        ra, rb = find(a[k]), find(b[k])
        if ra == rb:
            raise ValueError("edge %d closes a cycle: not a spanning tree" % k)
        node = n + k
        parent[ra] = parent[rb] = node
        size[node] = size[ra] + size[rb]
        left[k], right[k], sz[k] = ra, rb, size[node]
    return left, right, np.sqrt(np.asarray(mr2, dtype=np.float64)), sz


class Condensed:
    """pt_cluster / pt_lambda: every point's condensed-tree parent and the lambda at which it leaves it;
    cl_parent / cl_birth / cl_size: per condensed cluster (0 is the root: parent -1, birth 0)."""

    def __init__(self, pt_cluster, pt_lambda, cl_parent, cl_birth, cl_size):
        self.pt_cluster, self.pt_lambda = pt_cluster, pt_lambda
        self.cl_parent, self.cl_birth, self.cl_size = cl_parent, cl_birth, cl_size


def condense(tree, n, c):
    left, right, dist, size = tree
    left, right, size = left.tolist(), right.tolist(), size.tolist()
    with np.errstate(divide="ignore"):
        lam_of = np.where(dist > 0.0, 1.0 / dist, np.inf).tolist()
    root = 2 * n - 2
    cluster_of = [-1] * (2 * n - 1)         # the condensed cluster a single-linkage node belongs to; -1: fell out
    cluster_of[root] = 0
    pt_cluster = np.full(n, -1, dtype=np.int32)
    pt_lambda = np.zeros(n, dtype=np.float64)
    cl_parent, cl_birth, cl_size = [-1], [0.0], [n]

    def fall_out(node, cl, lam):
        stack = [node]
        while stack:
            x = stack.pop()
            if x < n:
                pt_cluster[x], pt_lambda[x] = cl, lam
            else:
                stack.append(left[x - n])
                stack.append(right[x - n])

    for node in range(root, n - 1, -1):
        cl = cluster_of[node]
        if cl < 0:
            continue
        l, r, lam = left[node - n], right[node - n], lam_of[node - n]
        lc = size[l - n] if l >= n else 1
        rc = size[r - n] if r >= n else 1
        if lc >= c and rc >= c:
            for child, count in ((l, lc), (r, rc)):
                cluster_of[child] = len(cl_parent)
                cl_parent.append(cl)
                cl_birth.append(lam)
                cl_size.append(count)
        elif lc < c and rc < c:
            fall_out(l, cl, lam)
            fall_out(r, cl, lam)
        elif lc < c:
            cluster_of[r] = cl
            fall_out(l, cl, lam)
        else:
            cluster_of[l] = cl
            fall_out(r, cl, lam)
    if n == 1:
        pt_cluster[0] = 0
    return Condensed(pt_cluster, pt_lambda, np.asarray(cl_parent, dtype=np.int32),
                     np.asarray(cl_birth, dtype=np.float64), np.asarray(cl_size, dtype=np.int64))


def stabilities(ct):
    """sum over a cluster's children (points: size 1, clusters: their size) of (lambda - birth) * size."""
    n_cl = ct.cl_parent.shape[0]
    stab = np.zeros(n_cl, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        np.add.at(stab, ct.pt_cluster, ct.pt_lambda - ct.cl_birth[ct.pt_cluster])
        if n_cl > 1:
            par = ct.cl_parent[1:]
            np.add.at(stab, par, (ct.cl_birth[1:] - ct.cl_birth[par]) * ct.cl_size[1:])
    return stab


def select_eom(ct):
    """bool per condensed cluster: selected.  Children before parents (a child's number is above its parent's); a
    cluster whose children's summed stability is greater hands that sum up, otherwise it is kept and everything
    below it is dropped.  The root is never a cluster."""
    stab = stabilities(ct).tolist()
    n_cl = len(stab)
    parent = ct.cl_parent.tolist()
    children = [[] for _ in range(n_cl)]
    for k in range(1, n_cl):
        children[parent[k]].append(k)
    selected = [True] * n_cl
    selected[0] = False
    for k in range(n_cl - 1, 0, -1):
        sub = 0.0
        for ch in children[k]:
            sub += stab[ch]
        if sub > stab[k]:
            selected[k] = False
            stab[k] = sub
        else:
            stack = list(children[k])
            while stack:
                x = stack.pop()
                selected[x] = False
                stack.extend(children[x])
    return np.asarray(selected, dtype=bool)


def labels(ct, selected):
    """(point labels int32 [n], cl_label int32 [n_cl]): a cluster at or below a selected one carries that one's
    label, every other -1; a point carries its parent's."""
    n_cl = ct.cl_parent.shape[0]
    anc = np.full(n_cl, -1, dtype=np.int64)
    for k in range(1, n_cl):
        anc[k] = k if selected[k] else anc[ct.cl_parent[k]]
    pt_anc = anc[ct.pt_cluster]
    cl_label = np.full(n_cl, -1, dtype=np.int32)
    seen = pt_anc >= 0
    if seen.any():
        idx = np.flatnonzero(seen)
        first = np.full(n_cl, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(first, pt_anc[idx], idx)
        order = [k for k in np.argsort(first, kind="stable").tolist() if selected[k] and first[k] < np.iinfo(np.int64).max]
        number = np.full(n_cl, -1, dtype=np.int32)
        number[order] = np.arange(len(order), dtype=np.int32)
        cl_label = np.where(anc >= 0, number[np.maximum(anc, 0)], -1).astype(np.int32)
    return cl_label[ct.pt_cluster].astype(np.int32), cl_label


class Tree:
    """What a fit keeps (include/ppk.h: ppk_dbscan_create)."""

    def __init__(self, labels, pt_cluster, pt_lambda, cl_parent, cl_birth, cl_label):
        self.labels = labels
        self.pt_cluster, self.pt_lambda = pt_cluster, pt_lambda
        self.cl_parent, self.cl_birth, self.cl_label = cl_parent, cl_birth, cl_label

    @property
    def n_clusters(self):
        return int(self.cl_label.max()) + 1 if self.cl_label.size else 0


def fit_tree(a, b, mr2, n, min_cluster_size):
    ct = condense(single_linkage(a, b, mr2, n), n, int(min_cluster_size))
    lab, cl_label = labels(ct, select_eom(ct))
    return Tree(lab, ct.pt_cluster, ct.pt_lambda, ct.cl_parent, ct.cl_birth, cl_label)


# ---- PopPUNK's glue -----------------------------------------------------------------------------------------------
def findWithinLabel(means, assignments, rank=0):
    """PopPUNK/bgmm.py:71-97: the label with the mean closest to the origin among those some sample carries."""
    dists = [(k, float(np.linalg.norm(mu))) for k, mu in enumerate(np.asarray(means))
             if np.any(np.asarray(assignments) == k)]
    dists.sort(key=lambda kv: kv[1])
    return dists[rank][0]


def findBetweenLabel(assignments, within_cluster):
    """PopPUNK/dbscan.py:98-123: the most frequent label that is neither noise nor the within-strain one (the first
    met in ascending label order among equally frequent ones; the reference's order there is a set's)."""
    y = np.asarray(assignments)
    y = y[(y != within_cluster) & (y != -1)]
    if y.size == 0:
        raise ValueError("no between-strain cluster: every point is noise or within-strain")
    vals, counts = np.unique(y, return_counts=True)
    return int(vals[np.argmax(counts)])


def evaluate_dbscan_clusters(cluster_mins, cluster_maxs, within_label, between_label):
    """PopPUNK/dbscan.py:69-96: True (indistinct) unless the between-strain cluster starts above the within-strain
    cluster's end in core or in accessory distance."""
    return not (cluster_mins[between_label, 0] > cluster_maxs[within_label, 0]
                or cluster_mins[between_label, 1] > cluster_maxs[within_label, 1])
