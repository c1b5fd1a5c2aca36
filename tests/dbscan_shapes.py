"""Input builders for the shapes of ppk_dbscan.hip that blob-shaped inputs never reach, and a numpy
restatement of the first square the grid search of the assignment tries for a row.  tests/test_dbscan_host.py proves
on the CPU what each builder claims; tests/test_gpu_dbscan_shapes.py runs them on the device.  Nothing here is a
reference for a label or a distance: those stay in tests/test_dbscan_host.py."""
import numpy as np


# ---- training points -------------------------------------------------------------------------------------------------
def two_chains(n):
    """float32 [n, 2]: two collinear chains of n // 2 and n - n // 2 points on the lines y = 0 and y = 64.  Inside a
    chain of `len` points, point i sits at x = 2^-20 * sum_{j<i} (len - j): the gaps strictly decrease, so at m = 1
    every point's least mutual-reachability edge under (mr2, lo, hi) goes to its successor (the last point's to its
    predecessor).  Round one of Boruvka then hooks a chain into one tree about len deep; round two joins the two only
    if every component id was compressed to its root.  Exact in float32 for n <= 4096."""
    assert 4 <= n <= 4096
    out = []
    for length, y in ((n // 2, 0.0), (n - n // 2, 64.0)):
        gaps = length - np.arange(length - 1, dtype=np.int64)
        x = np.concatenate([[0], np.cumsum(gaps)]).astype(np.float64) * 2.0 ** -20
        out.append(np.stack([x, np.full(length, y)], axis=1))
    P64 = np.vstack(out)
    P = P64.astype(np.float32)
    assert np.array_equal(P.astype(np.float64), P64)          # the round trip: every coordinate is a float32
    return P


def lattice(s):
    """float32 [s * s, 2]: the s x s integer lattice divided by 32, row by row.  Every d2 is a small integer over
    1024, so core distances and edge weights tie exactly in large groups."""
    i = np.arange(s, dtype=np.float32) / np.float32(32.0)
    return np.stack([np.tile(i, s), np.repeat(i, s)], axis=1).astype(np.float32)


def wide_range(n, seed):
    """float32 [n, 2]: coordinates +-2^e * u, e a uniform integer in [-60, 60], u uniform in [1, 2).  The d2 of such
    points span more than 200 binades, so the two-bit selection takes every branch in its exponent passes."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-60, 61, (n, 2))
    u = rng.uniform(1.0, 2.0, (n, 2))
    sign = np.where(rng.integers(0, 2, (n, 2)) == 1, 1.0, -1.0)
    return (sign * np.ldexp(u, e)).astype(np.float32)


def least_partner(P, core2):
    """int [n]: for every point the other end of its least edge under (mr2, lo, hi).  For one point the order of its
    edges by (lo, hi) is the order of the partner's index, so it is the first partner at the least mr2."""
    P64 = np.asarray(P, dtype=np.float32).astype(np.float64)
    dx, dy = P64[:, None, 0] - P64[None, :, 0], P64[:, None, 1] - P64[None, :, 1]
    mr2 = dx * dx
    del dx
    mr2 += dy * dy
    del dy
    np.maximum(mr2, core2[:, None], out=mr2)
    np.maximum(mr2, core2[None, :], out=mr2)
    np.fill_diagonal(mr2, np.inf)
    return np.argmin(mr2, axis=1)


def chain_successors(n):
    """What least_partner must give on two_chains(n) at m = 1: i + 1, and i - 1 for the last point of a chain."""
    want = np.arange(n) + 1
    want[n // 2 - 1] = n // 2 - 2
    want[n - 1] = n - 2
    return want


# ---- the grid of ppk_dbscan_create and a row's first square ----------------------------------------------------------
class Grid:
    """g, the origin (x0, y0), the cell widths (wx, wy), eps, every training point's cell (cx, cy), the points as
    float64 and the g x g table of cell counts (count[cy, cx])."""


def grid_of(P):
    P = np.ascontiguousarray(P, dtype=np.float32)
    G = Grid()
    G.P64 = P.astype(np.float64)
    G.n = n = len(P)
    G.g = g = min(max(int(np.sqrt(n / 4.0)), 1), 1024)
    x0, y0 = G.P64.min(axis=0)
    x1, y1 = G.P64.max(axis=0)
    G.x0, G.y0 = float(x0), float(y0)
    G.wx = float((x1 - x0) / g) if x1 > x0 else 1.0
    G.wy = float((y1 - y0) / g) if y1 > y0 else 1.0
    G.eps = 1e-9 * max(G.wx, G.wy) * g
    G.cx = np.clip(np.floor((G.P64[:, 0] - G.x0) / G.wx).astype(np.int64), 0, g - 1)
    G.cy = np.clip(np.floor((G.P64[:, 1] - G.y0) / G.wy).astype(np.int64), 0, g - 1)
    G.count = np.zeros((g, g), dtype=np.int64)
    np.add.at(G.count, (G.cy, G.cx), 1)
    # count of the cells [0, cy) x [0, cx): any square's count in four reads
    G.cum = np.zeros((g + 1, g + 1), dtype=np.int64)
    G.cum[1:, 1:] = G.count.cumsum(axis=0).cumsum(axis=1)
    return G


def _cell(f, g):
    return (int(f) if f < g else g - 1) if f >= 0.0 else 0          # a NaN lands in cell 0


def _first_square_cells(G, q, m):
    g, n = G.g, G.n
    cxq, cyq = _cell((float(q[0]) - G.x0) / G.wx, g), _cell((float(q[1]) - G.y0) / G.wy, g)
    need = min(2 * m, n)
    target = min(need + need // 2 + 8, n)
    r = 0
    while True:
        cx0, cy0 = max(cxq - r, 0), max(cyq - r, 0)
        cx1, cy1 = min(cxq + r, g - 1), min(cyq + r, g - 1)
        is_all = cx0 == 0 and cy0 == 0 and cx1 == g - 1 and cy1 == g - 1
        if is_all or square_count(G, cx0, cx1, cy0, cy1) >= target:
            return cx0, cx1, cy0, cy1, is_all, need, target
        r += 1 + r // 4


def square_count(G, cx0, cx1, cy0, cy1):
    return int(G.cum[cy1 + 1, cx1 + 1] - G.cum[cy0, cx1 + 1] - G.cum[cy1 + 1, cx0] + G.cum[cy0, cx0])


def first_square(G, q, m):
    """The first attempt of dbscan_assign_grid_kernel for the scaled float64 row q: the row's cell; need = min(2m, n)
    and target = min(need + need // 2 + 8, n); the square around the cell grown by r += 1 + r // 4 until it holds
    `target` points or is the whole grid; dk2, the need-th smallest d2 inside it; the margin to the nearest side with
    cells beyond it and safe = margin * (1 - 1e-9) - eps.  The same uncontracted double arithmetic as the kernel.
    Returns (grid_rows, grid_cols, is_all, dk2, safe); the row certifies at once when safe > 0 and dk2 < safe^2.
    This picks the rows a test plants.  It is no reference for labels."""
    g = G.g
    qx, qy = float(q[0]), float(q[1])
    cx0, cx1, cy0, cy1, is_all, need, _ = _first_square_cells(G, q, m)
    inside = (G.cx >= cx0) & (G.cx <= cx1) & (G.cy >= cy0) & (G.cy <= cy1)
    dx, dy = qx - G.P64[inside, 0], qy - G.P64[inside, 1]
    d2 = dx * dx + dy * dy
    dk2 = float(np.partition(d2, need - 1)[need - 1])
    margin = np.inf
    if cx0 > 0:
        margin = min(margin, qx - (G.x0 + float(cx0) * G.wx))
    if cx1 < g - 1:
        margin = min(margin, (G.x0 + float(cx1 + 1) * G.wx) - qx)
    if cy0 > 0:
        margin = min(margin, qy - (G.y0 + float(cy0) * G.wy))
    if cy1 < g - 1:
        margin = min(margin, (G.y0 + float(cy1 + 1) * G.wy) - qy)
    safe = margin * (1.0 - 1e-9) - G.eps
    return cy1 - cy0 + 1, cx1 - cx0 + 1, is_all, dk2, safe


def rows_past_the_64th_decide(G, q, m):
    """True when the first 64 grid rows of q's first square hold fewer points than the target on their own: the
    square stops growing where it does only because the count's second strided run adds the grid rows past them."""
    cx0, cx1, cy0, cy1, is_all, _, target = _first_square_cells(G, q, m)
    return not is_all and cy1 - cy0 + 1 > 64 and square_count(G, cx0, cx1, cy0, cy0 + 63) < target


def regrown_square_is_all(G, dk2):
    """After a first square that did not certify the kernel regrows it once from the distance found, and takes the
    whole grid when the radius that asks for is no less than g."""
    rr = (np.sqrt(dk2) * (1.0 + 1e-9) + 2.0 * G.eps) / min(G.wx, G.wy) + 2.0
    return not rr < float(G.g)


# ---- the grid of more than 64 rows -----------------------------------------------------------------------------------
FAR_ROWS = np.array([[30.0, 30.0], [-5.0, 0.5], [0.5, 1e6], [1e-30, -1e4]], dtype=np.float32)
NON_FINITE_ROWS = np.array([[np.inf, 0.5], [np.nan, 0.2]], dtype=np.float32)
TALL_M = 1023


def tall_grid_points(blob="low"):
    """20 000 training points, g = 70: a dense blob in one corner and a thin uniform background, so that a row in
    the background needs a square of most of the grid to collect 1.5 x 2m points; and 4 000 rows in the background.
    "low": the blob at (0.15, 0.15), in the first grid rows of such a square.  "top": the blob against the upper edge,
    in the grid rows past the square's 64th, which only the second run of the lanes' strided count reaches."""
    if blob == "low":
        rng = np.random.default_rng(31)
        P = np.vstack([np.abs(rng.normal([0.15, 0.15], 0.02, (18500, 2))), rng.uniform(0, 1, (1500, 2))])
        rows = rng.uniform(0.3, 0.95, (4000, 2))
    else:
        rng = np.random.default_rng(33)
        P = np.vstack([np.abs(rng.normal([0.15, 0.03], 0.02, (18500, 2))), rng.uniform(0, 1, (1500, 2))])
        P[:, 1] = 1.0 - P[:, 1]
        rows = rng.uniform([0.3, 0.05], [0.95, 0.7], (4000, 2))
    return P.astype(np.float32), rows.astype(np.float32)


def scanned_far_rows(G, m):
    """The FAR_ROWS that end as a scan of everything: the first square is the whole grid, or it fails to certify by
    10 % or more and the radius asked for next is no less than g."""
    out = []
    for i, q in enumerate(FAR_ROWS.astype(np.float64)):
        _, _, is_all, dk2, safe = first_square(G, q, m)
        if is_all or (not (safe > 0.0 and dk2 < 1.1 * safe * safe) and regrown_square_is_all(G, dk2)):
            out.append(i)
    return out


def tall_grid_row_sets(G, rows, m, scale=None, first=1500):
    """Of rows[:first]: set A, the rows whose first square spans more than 64 grid rows, is not the whole grid and
    certifies with dk2 < 0.9 * safe^2 (they are never scanned); the rows whose first square spans more than 64 grid
    rows and is not the whole grid, certified or not; and the rows whose first square is the whole grid (they are
    counted as scanned)."""
    A, tall, whole = [], [], []
    for i in range(first):
        q = rows[i].astype(np.float64) if scale is None else rows[i].astype(np.float64) / scale
        gr, _, is_all, dk2, safe = first_square(G, q, m)
        if is_all:
            whole.append(i)
        elif gr > 64:
            tall.append(i)
            if safe > 0.0 and dk2 < 0.9 * safe * safe:
                A.append(i)
    return np.array(A, dtype=np.int64), np.array(tall, dtype=np.int64), np.array(whole, dtype=np.int64)


# ---- a model without a fit -------------------------------------------------------------------------------------------
class SyntheticModel:
    """The arrays DBSCANModel._set_state and the assignment restatement read, drawn rather than fitted."""

    @property
    def n_clusters(self):
        return int(self.cl_label.max()) + 1


def synthetic_model(n_points, n_cl, rng, points=None):
    """A model the assignment takes as it stands, with no O(n^2) fit: core2 random and positive over the points' d2
    scale; cl_parent[k] = k - 1 for the first half of the clusters (a deep chain) and a random earlier cluster for
    the rest; random positive births and leaving lambdas over the scale of 1 / sqrt(d2); labels from -1 to 4; every
    point in a random cluster.  `points` (float32 [n_points, 2]) are drawn uniform in [0, 1]^2 when not given."""
    assert 1 <= n_cl <= n_points
    M = SyntheticModel()
    if points is None:
        points = rng.uniform(0, 1, (n_points, 2))
    M.points = np.ascontiguousarray(points, dtype=np.float32)
    assert M.points.shape == (n_points, 2)
    M.core2 = np.exp(rng.uniform(np.log(1e-7), np.log(1.0), n_points))
    half = n_cl // 2
    parent = np.empty(n_cl, dtype=np.int32)
    parent[0] = -1
    for k in range(1, n_cl):
        parent[k] = k - 1 if k <= half else rng.integers(0, k)
    M.cl_parent = parent
    M.cl_birth = np.exp(rng.uniform(np.log(0.5), np.log(1e4), n_cl))
    M.cl_birth[0] = 0.0
    M.cl_label = rng.integers(-1, 5, n_cl).astype(np.int32)
    M.cl_label[:6] = [-1, 0, 1, 2, 3, 4]
    M.pt_cluster = rng.integers(0, n_cl, n_points).astype(np.int32)
    M.pt_cluster[:min(n_cl, n_points)] = np.arange(min(n_cl, n_points))[::-1]     # every depth of the chain is a start
    M.pt_lambda = np.exp(rng.uniform(np.log(0.5), np.log(1e4), n_points))
    M.labels = M.cl_label[M.pt_cluster]
    return M


def walk_depth(q, M, m):
    """How many clusters the assignment of the scaled float64 row q climbs (tests/test_dbscan_host.py: ref_assign_row)."""
    P64 = M.points.astype(np.float64)
    n = len(P64)
    dx, dy = q[0] - P64[:, 0], q[1] - P64[:, 1]
    d2 = dx * dx + dy * dy
    order = np.lexsort((np.arange(n), d2))
    N = order[:min(2 * m, n)]
    w = np.maximum(np.maximum(M.core2[N], d2[order[min(m, n - 1)]]), d2[N])
    j = int(np.argmin(w))
    lq = 1.0 / np.sqrt(w[j]) if w[j] > 0.0 else np.finfo(np.float64).max
    cl, depth = int(M.pt_cluster[N[j]]), 0
    if M.pt_lambda[N[j]] > lq:
        while cl != 0 and M.cl_birth[cl] >= lq:
            cl, depth = int(M.cl_parent[cl]), depth + 1
    return depth
