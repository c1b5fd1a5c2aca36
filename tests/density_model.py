"""The two rules of the density grids (include/ppk.h "Density grids") restated in numpy, integer
accumulation included: what ppk_density_kde* and ppk_density_counts* must give bit for bit.  Dense on purpose: every
row meets every cell, no window."""
import numpy as np

H = 0.03            # plot_scatter's bandwidth (PopPUNK/plot.py:62)


def load_golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density.npz"))


def scaled(dist, scale, idx=None):
    """px, py of the rows read: float32 divisions, then widened."""
    x = np.asarray(dist, dtype=np.float32).reshape(-1, 2)
    if idx is not None:
        x = x[np.asarray(idx, dtype=np.int64)]
    s = np.asarray(scale, dtype=np.float32)
    return (x[:, 0] / s[0]).astype(np.float64), (x[:, 1] / s[1]).astype(np.float64)


def kde_sums(dist, gx, gy, h, scale, shift, idx=None, block=None):
    """(sum int64 [nx, ny], cnt int64 [nx, ny]): the fixed-point sums and how many rows reach each cell."""
    gx, gy = np.asarray(gx, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    px, py = scaled(dist, scale, idx)
    inv_h2 = 1.0 / (h * h)
    fix = 2.0 ** shift
    total = np.zeros((len(gx), len(gy)), dtype=np.int64)
    cnt = np.zeros((len(gx), len(gy)), dtype=np.int64)
    block = block or max(1, 4_000_000 // (len(gx) * len(gy)))
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, len(px), block):
            dx = px[lo:lo + block, None] - gx[None, :]
            dy = py[lo:lo + block, None] - gy[None, :]
            d2 = (dx * dx)[:, :, None] + (dy * dy)[:, None, :]
            t = 1.0 - d2 * inv_h2
            hit = t > 0
            total += np.where(hit, np.rint(t * fix), 0.0).astype(np.int64).sum(axis=0)
            cnt += hit.sum(axis=0)
    return total, cnt


def kde_norm(h, n):
    """sklearn's normalisation of the 2-D Epanechnikov kernel: z = sum * 2^-shift * kde_norm."""
    return 2.0 / (np.pi * h * h * n)


def z_from_sums(total, shift, h, n):
    """The reference's z (z.reshape(xx.shape).T: [accessory node, core node]) from sums [core node, accessory node]."""
    return (np.asarray(total, dtype=np.float64) * 2.0 ** -shift * kde_norm(h, n)).T


def counts(dist, raster, labels=None, label_lo=0, n_slots=1):
    """(counts uint32 [n_slots, ny, nx], outside)."""
    x0, inv_dx, nx, y0, inv_dy, ny = raster
    x = np.asarray(dist, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    fx = np.floor((x[:, 0] - x0) * inv_dx)
    fy = np.floor((x[:, 1] - y0) * inv_dy)
    inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
    slot = np.zeros(len(x), dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64) - label_lo
    assert np.all((slot >= 0) & (slot < n_slots))
    cell = (slot[inside] * ny + fy[inside].astype(np.int64)) * nx + fx[inside].astype(np.int64)
    out = np.bincount(cell, minlength=n_slots * ny * nx).astype(np.uint32).reshape(n_slots, ny, nx)
    return out, int(len(x) - inside.sum())


def shuffle_indices(n, seed, keep):
    """The rows sklearn.utils.shuffle(X, random_state=seed)[0:keep] holds (utils.resample: RandomState(seed).shuffle
    of arange(n))."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    return idx[:keep]
