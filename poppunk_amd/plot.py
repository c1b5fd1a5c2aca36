"""The distance-distribution and model-fit plots of PopPUNK/plot.py on the MI355X.

Mirrors the reference's names, arguments, file names, titles and labels for
  * `get_grid`, `plot_scatter`                      PopPUNK/plot.py:31-82, :416-441
  * `plot_results`, `plot_contours`                 :182-235, :375-414 (BGMMFit.plot)
  * `plot_dbscan_results`                           :237-283
  * `plot_refined_results`                          :285-373 (RefineFit.plot)
  * `distHistogram`                                 :443-466
Every X (and Y) is a numpy array or a resident CUDA tensor.  Both layers of these pictures reduce the matrix to a small
grid, and the grids are made on the device:
  * the kernel density behind plot_scatter's contours is `engine.density_kde*` over EVERY row (`scatter_density`);
  * the scatter layer is the reference's own one-marker-per-row call up to `raster_above` rows (default 1 000 000), and
    above that one `imshow` of the per-label occupancy raster (`engine.density_counts*`) at the figure's pixel size,
    11 x 8 in at 160 dpi.  Where labels overlap in a pixel the label the reference draws last wins: the highest
    component index for BGMM, clusters over noise for DBSCAN, between-strain over within-strain for refine.
Each picture is a pure data function (`scatter_density`, `scatter_points`, `label_raster`, `raster_image`,
`contour_surfaces`), which the tests check, and a thin drawing function.  matplotlib is imported inside the drawing
functions, with the Agg backend, so the package imports without it.
"""
import itertools
import os
import random
import sys

import numpy as np

from . import engine

KDE_BANDWIDTH = 0.03                 # plot.py:62
KDE_RESOLUTION = 100                 # plot.py:59
FIGSIZE, DPI = (11, 8), 160          # every figure of the reference
RASTER_NX, RASTER_NY = FIGSIZE[0] * DPI, FIGSIZE[1] * DPI      # 1760 x 1280
RASTER_MARGIN = 0.05                 # matplotlib's default axes margin around the data
BGMM_COLOURS = ['navy', 'c', 'cornflowerblue', 'gold', 'darkorange']      # plot.py:207


def _pyplot():
    """(matplotlib, matplotlib.pyplot) with the reference's backend and font size (plot.py:11-14)."""
    import matplotlib as mpl
    mpl.use('Agg')
    mpl.rcParams.update({'font.size': 18})
    import matplotlib.pyplot as plt
    return mpl, plt


def _is_tensor(a):
    return hasattr(a, "is_cuda")


def _host(a):
    return a.cpu().numpy() if _is_tensor(a) else np.asarray(a)


def _rows(X):
    return int(X.shape[0])


def get_grid(minimum, maximum, resolution):
    """plot.py:416-441: xx, yy of np.meshgrid and the points [yy.ravel(), xx.ravel()] the functions are evaluated on."""
    x = np.linspace(minimum, maximum, resolution)
    y = np.linspace(minimum, maximum, resolution)
    xx, yy = np.meshgrid(x, y)
    xy = np.vstack([yy.ravel(), xx.ravel()]).T
    return (xx, yy, xy)


def shuffle_indices(n, seed, keep):
    """The rows `sklearn.utils.shuffle(X, random_state=seed)[0:keep]` holds, restated: utils.resample shuffles
    np.arange(n) with numpy.random.RandomState(seed) and takes the rows in that order."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    return idx[:keep]


class ScatterDensity:
    """What plot_scatter draws its contours from: scale (float32 [2]), xx, yy, z ([accessory node, core node], the
    reference's `z.reshape(xx.shape).T`), levels (all ten: the reference passes levels[1:]), idx (the sampled rows, or
    None: every row), rows_read and the fixed-point shift of the sums."""

    def __init__(self, scale, xx, yy, z, levels, idx, rows_read, shift, sums):
        self.scale, self.xx, self.yy, self.z, self.levels = scale, xx, yy, z, levels
        self.idx, self.rows_read, self.shift, self.sums = idx, rows_read, shift, sums


def scatter_density(X, kde_rows="all", max_plot_samples=1000000, seed=None):
    """scale, xx, yy, z and levels as plot.py:54-68 forms them, with the density from the device:
    z = sum * 2^-shift * 2 / (pi h^2 N), sklearn's normalisation of the 2-D Epanechnikov kernel, on get_grid(0, 1, 100).

    kde_rows="all" reads every row.  On matrices of at most max_plot_samples rows that is what the reference computes;
    above that the reference fits a random sample of max_plot_samples rows, and using every row instead is this
    project's choice [EXT-deviation].  kde_rows="sample" reproduces the reference there: the rows
    sklearn.utils.shuffle(X, random_state=seed) keeps (`shuffle_indices`; seed None draws random.randint(1, 10000) as
    the reference does), as an index list the kernel reads -- the matrix is not copied.  scale is the column maxima of
    the rows read, float32, as np.amax gives them.

    The reference's `X /= scale` divides the caller's array in place; nothing here writes to X."""
    if kde_rows not in ("all", "sample"):
        raise ValueError("kde_rows must be 'all' or 'sample'")
    n = _rows(X)
    idx = None
    if kde_rows == "sample" and n > max_plot_samples:
        if seed is None:
            seed = random.randint(1, 10000)
        idx = shuffle_indices(n, seed, max_plot_samples)
    xx, yy, _ = get_grid(0, 1, KDE_RESOLUTION)
    g = np.linspace(0, 1, KDE_RESOLUTION)
    if _is_tensor(X):
        import torch
        idx_t = None if idx is None else torch.as_tensor(idx, dtype=torch.int64, device=X.device)
        sums_t, shift, rows_read, scale = engine.density_kde_dev(X, g, g, KDE_BANDWIDTH, idx_t=idx_t, return_scale=True)
        sums = sums_t.cpu().numpy()
    else:
        sums, shift, rows_read, scale = engine.density_kde(X, g, g, KDE_BANDWIDTH, idx=idx)
    z = kde_values(sums, shift, KDE_BANDWIDTH, rows_read)
    levels = np.linspace(z.min(), z.max(), 10)
    return ScatterDensity(scale, xx, yy, z, levels, idx, rows_read, shift, sums)


def kde_values(sums, shift, h, n):
    """The density in the reference's orientation from the sums [core node, accessory node]."""
    return (np.asarray(sums, dtype=np.float64) * 2.0 ** -shift * (2.0 / (np.pi * h * h * n))).T


def scatter_points(X, scale, idx=None):
    """plot_scatter's two scatter arguments (plot.py:55, :76): (X / scale) * scale column by column in float32 -- not
    always X's own bits."""
    if idx is None:
        x = _host(X)
    elif _is_tensor(X):
        x = _host(X[_index_tensor(X, idx)])
    else:
        x = np.asarray(X)[np.asarray(idx)]
    x = np.asarray(x, dtype=np.float32)
    s = np.asarray(scale, dtype=np.float32)
    xs = x / s
    return xs[:, 0] * s[0:1], xs[:, 1] * s[1:2]


def _take_rows(X, idx):
    return X[_index_tensor(X, idx)] if _is_tensor(X) else np.asarray(X)[np.asarray(idx)]


def _index_tensor(X, idx):
    import torch
    return torch.as_tensor(np.asarray(idx), dtype=torch.int64, device=X.device)


def column_max(X):
    """np.amax(X, axis=0) of either kind of matrix, as float64 [2]."""
    if _is_tensor(X):
        return X.amax(dim=0).cpu().numpy().astype(np.float64)
    return np.amax(np.asarray(X), axis=0).astype(np.float64)


def raster_for(xy_max, nx=RASTER_NX, ny=RASTER_NY, margin=RASTER_MARGIN):
    """The raster (x0, inv_dx, nx, y0, inv_dy, ny) and the imshow extent of a picture whose data lie in [0, xy_max]:
    matplotlib's margin on both sides."""
    mx, my = (float(v) if v > 0 else 1.0 for v in xy_max)
    x0, x1 = -margin * mx, (1.0 + margin) * mx
    y0, y1 = -margin * my, (1.0 + margin) * my
    return (x0, nx / (x1 - x0), nx, y0, ny / (y1 - y0), ny), (x0, x1, y0, y1)


def label_raster(X, Y=None, label_lo=0, n_slots=1, raster=None):
    """(counts uint32 [n_slots, ny, nx] numpy, outside, extent): the occupancy of the figure's pixels per label."""
    extent = None
    if raster is None:
        raster, extent = raster_for(column_max(X))
    if _is_tensor(X):
        import torch
        lab = None
        if Y is not None:
            lab = Y if _is_tensor(Y) else torch.as_tensor(np.asarray(Y), device=X.device)
            lab = lab.to(dtype=torch.int32).contiguous()
        counts_t, outside_t = engine.density_counts_dev(X, raster, lab, label_lo, n_slots)
        counts, outside = counts_t.cpu().numpy(), int(outside_t.cpu()[0])
    else:
        counts, outside = engine.density_counts(X, raster, None if Y is None else _host(Y), label_lo, n_slots)
    return counts, outside, extent


MAX_SLOTS, MAX_COUNT_CELLS = 32, 1 << 26      # labels, and labels x pixels, one ppk_density_counts* call takes


def label_rasters(X, Y, label_lo, n_labels, raster=None):
    """label_raster for any number of labels: labels label_lo .. label_lo + n_labels - 1 in passes of as many labels as
    one call takes (at most MAX_SLOTS, and MAX_COUNT_CELLS cells: 29 at the figure's size).  A pass counts the rows
    of its own labels, so `outside` is taken from a pass without labels.  Returns (counts uint32 [n_labels, ny, nx],
    outside, extent); ValueError for a label outside the range."""
    extent = None
    if raster is None:
        raster, extent = raster_for(column_max(X))
    per = max(1, min(MAX_SLOTS, MAX_COUNT_CELLS // (raster[2] * raster[5])))
    if n_labels <= per:
        counts, outside, _ = label_raster(X, Y, label_lo, n_labels, raster=raster)
        return counts, outside, extent
    _, outside, _ = label_raster(X, raster=raster)
    parts, kept = [], 0
    for lo in range(label_lo, label_lo + n_labels, per):
        n = min(per, label_lo + n_labels - lo)
        if _is_tensor(X):
            Yt = Y if _is_tensor(Y) else _index_tensor(X, Y)
            keep = (Yt >= lo) & (Yt < lo + n)
            c, _, _ = label_raster(X[keep].contiguous(), Yt[keep], lo, n, raster=raster)
        else:
            Yh = _host(Y)
            keep = (Yh >= lo) & (Yh < lo + n)
            c, _, _ = label_raster(np.asarray(X)[keep], Yh[keep], lo, n, raster=raster)
        parts.append(c)
        kept += int(keep.sum())
    if kept != _rows(X):
        raise ValueError("%d labels outside [%d, %d)" % (_rows(X) - kept, label_lo, label_lo + n_labels))
    return np.concatenate(parts, axis=0), outside, extent


def raster_image(counts, colours):
    """An RGBA float image [ny, nx, 4] from per-slot counts: `colours` is a list of (slot, rgba) in drawing order, so a
    later entry overwrites an earlier one where both hold a row; pixels without a row stay transparent."""
    img = np.zeros(counts.shape[1:] + (4,), dtype=np.float32)
    for slot, rgba in colours:
        img[counts[slot] > 0] = np.asarray(rgba, dtype=np.float32)
    return img


def _draw_raster(plt, mpl, counts, colours, extent, outside):
    img = raster_image(counts, [(s, mpl.colors.to_rgba(c)) for s, c in colours])
    plt.imshow(img, extent=extent, origin='lower', aspect='auto', interpolation='nearest')
    if outside:
        sys.stderr.write("%d rows lie outside the plotted range\n" % outside)


def _axis_labels(plt, title):
    plt.title(title)
    plt.xlabel('Core distance (' + r'$\pi$' + ')')
    plt.ylabel('Accessory distance (' + r'$a$' + ')')


def plot_scatter(X, out_prefix, title, kde=True, raster_above=1000000, kde_rows="all", seed=None):
    """plot.py:31-82: the distance distribution with the contours of its kernel density, written to
    <out_prefix>/<basename>_distanceDistribution.png.  X is left as it was (the reference divides it by its maxima)."""
    mpl, plt = _pyplot()
    n = _rows(X)
    plt.figure(figsize=FIGSIZE, dpi=DPI, facecolor='w', edgecolor='k')
    idx = None
    if kde:
        sd = scatter_density(X, kde_rows=kde_rows, seed=seed)
        scale, idx = sd.scale, sd.idx
        plt.contour(sd.xx * scale[0], sd.yy * scale[1], sd.z, levels=sd.levels[1:], cmap='plasma')
        scatter_alpha = 1
    else:
        scale = None
        scatter_alpha = 0.1
    shown = n if idx is None else len(idx)
    if shown <= raster_above:
        if scale is None:
            scale = column_max(X).astype(np.float32)
        px, py = scatter_points(X, scale, idx)
        plt.scatter(px, py, s=1, alpha=scatter_alpha)
    else:
        counts, outside, extent = label_raster(X if idx is None else _take_rows(X, idx))      # the rows the points route draws
        _draw_raster(plt, mpl, counts, [(0, mpl.colors.to_rgba('C0', alpha=scatter_alpha))], extent, outside)
    _axis_labels(plt, title)
    plt.savefig(os.path.join(out_prefix, os.path.basename(out_prefix) + '_distanceDistribution.png'))
    plt.close()


def _label_counts(Y, lo, n_slots):
    """Rows per label lo .. lo + n_slots - 1."""
    if _is_tensor(Y):
        import torch
        y = (Y.to(torch.int64) - (lo - 1)).clamp_(0, n_slots + 1)         # labels out of range: bins 0 and n_slots + 1
        return torch.bincount(y, minlength=n_slots + 2)[1:n_slots + 1].cpu().numpy()
    y = np.asarray(Y).astype(np.int64) - lo
    return np.bincount(y[(y >= 0) & (y < n_slots)], minlength=n_slots)[:n_slots]


def plot_results(X, Y, means, covariances, scale, title, out_prefix, raster_above=1000000):
    """plot.py:182-235: the BGMM fit -- rows coloured by component, an ellipse per used component -- written to
    <out_prefix>.png."""
    mpl, plt = _pyplot()
    K = len(means)
    used = _label_counts(Y, 0, K) > 0
    raster = _rows(X) > raster_above
    plt.figure(figsize=FIGSIZE, dpi=DPI, facecolor='w', edgecolor='k')
    splot = plt.subplot(1, 1, 1)
    if raster:
        counts, outside, extent = label_rasters(X, Y, 0, K)
        colours = [(i, c) for i, c in zip(range(K), itertools.cycle(BGMM_COLOURS)) if used[i]]
        _draw_raster(plt, mpl, counts, colours, extent, outside)
    else:
        Xh, Yh = _host(X), _host(Y)
    scale = np.asarray(scale, dtype=np.float64)
    for i, (mean, covar, color) in enumerate(zip(means, covariances, itertools.cycle(BGMM_COLOURS))):
        scaled_covar = np.matmul(np.matmul(np.diag(scale), covar), np.diag(scale).T)
        v, w = np.linalg.eigh(scaled_covar)
        v = 2. * np.sqrt(2.) * np.sqrt(v)
        u = w[0] / np.linalg.norm(w[0])
        if not used[i]:
            continue
        if not raster:
            plt.scatter([(Xh)[Yh == i, 0]], [(Xh)[Yh == i, 1]], .4, color=color)
        angle = np.arctan(u[1] / u[0])
        angle = 180. * angle / np.pi
        ell = mpl.patches.Ellipse(mean * scale, v[0], v[1], angle=180. + angle, color=color)
        ell.set_clip_box(splot.bbox)
        ell.set_alpha(0.5)
        splot.add_artist(ell)
    _axis_labels(plt, title)
    plt.savefig(out_prefix + ".png")
    plt.close()


def plot_dbscan_results(X, y, n_clusters, out_prefix, use_gpu=False, raster_above=1000000):
    """plot.py:237-283: the DBSCAN fit -- noise in black, drawn first, each cluster in a colour of the Spectral map --
    written to <out_prefix>.png.  `use_gpu` is accepted for the signature: a CUDA tensor is recognised by itself."""
    mpl, plt = _pyplot()
    hi = max(int(n_clusters), 1)
    present = _label_counts(y, -1, hi + 1) > 0
    unique_labels = [k - 1 for k in range(hi + 1) if present[k]]           # noise first, then ascending
    colours = [plt.cm.Spectral(each) for each in np.linspace(0, 1, len(unique_labels))]
    plt.figure(figsize=FIGSIZE, dpi=DPI, facecolor='w', edgecolor='k')
    order = []
    for k in unique_labels:
        if k == -1:
            ptsize, col = 1, 'k'
        else:
            ptsize, col = 2, tuple(colours.pop())
        order.append((k, ptsize, col))
    if _rows(X) > raster_above:
        counts, outside, extent = label_rasters(X, y, -1, hi + 1)
        _draw_raster(plt, mpl, counts, [(k + 1, col) for k, _, col in order], extent, outside)
    else:
        Xh, yh = _host(X), _host(y)
        for k, ptsize, col in order:
            xy = Xh[yh == k]
            plt.plot(xy[:, 0], xy[:, 1], '.', color=col, markersize=ptsize)
    _axis_labels(plt, 'HDBSCAN – estimated number of spatial clusters: %d' % n_clusters)
    plt.savefig(out_prefix + ".png")
    plt.close()


def plot_refined_results(X, Y, x_boundary, y_boundary, core_boundary, accessory_boundary, mean0, mean1, min_move,
                         max_move, scale, threshold, indiv_boundaries, unconstrained, title, out_prefix,
                         raster_above=1000000):
    """plot.py:285-373: the refined fit -- within-strain rows (-1) and between-strain rows (1), the boundary, the
    individual boundaries and the search range -- written to <out_prefix>.png.  mean0 and mean1 are left as they were
    (the reference multiplies them by scale in place)."""
    from .utils import decisionBoundary, transformLine
    mpl, plt = _pyplot()
    plt.figure(figsize=FIGSIZE, dpi=DPI, facecolor='w', edgecolor='k')
    xy_max = column_max(X)
    if _rows(X) > raster_above:
        counts, outside, extent = label_raster(X, Y, -1, 3)
        _draw_raster(plt, mpl, counts, [(0, 'cornflowerblue'), (2, 'c')], extent, outside)
    else:
        Xh, Yh = _host(X), _host(Y)
        plt.scatter([(Xh)[Yh == -1, 0]], [(Xh)[Yh == -1, 1]], .4, color='cornflowerblue')
        plt.scatter([(Xh)[Yh == 1, 0]], [(Xh)[Yh == 1, 1]], .4, color='c')
    scale = np.asarray(scale, dtype=np.float64)
    if not threshold:
        plt.plot([x_boundary * scale[0], 0], [0, y_boundary * scale[1]], color='red', linewidth=2, linestyle='--',
                 label='Combined decision boundary')
        if indiv_boundaries:
            plt.plot([core_boundary * scale[0], core_boundary * scale[0]], [0, xy_max[1]], color='darkgray',
                     linewidth=1, linestyle='-.', label='Individual decision boundaries')
            plt.plot([0, xy_max[0]], [accessory_boundary * scale[1], accessory_boundary * scale[1]], color='darkgray',
                     linewidth=1, linestyle='-.')
        if mean0 is not None and mean1 is not None and min_move is not None and max_move is not None:
            mean0 = np.array(mean0, dtype=np.float64)
            mean1 = np.array(mean1, dtype=np.float64)
            if unconstrained:
                gradient = (mean1[1] - mean0[1]) / (mean1[0] - mean0[0])
                opt_start = decisionBoundary(mean0, gradient) * scale
                opt_end = decisionBoundary(mean1, gradient) * scale
                plt.fill([opt_start[0], opt_end[0], 0, 0], [0, 0, opt_end[1], opt_start[1]], fill=True,
                         facecolor='lightcoral', alpha=0.2, label='Search range')
            else:
                search_length = max_move + ((mean1[0] - mean0[0])**2 + (mean1[1] - mean0[1])**2)**0.5
                minimum_xy = transformLine(-min_move, mean0, mean1) * scale
                maximum_xy = transformLine(search_length, mean0, mean1) * scale
                plt.plot([minimum_xy[0], maximum_xy[0]], [minimum_xy[1], maximum_xy[1]], color='k', linewidth=1,
                         linestyle=':', label='Search range')
            mean0 = mean0 * scale
            mean1 = mean1 * scale
            plt.plot(mean0[0], mean0[1], 'rx', label='Within-strain mean')
            plt.plot(mean1[0], mean1[1], 'r+', label='Between-strain mean')
    else:
        plt.plot([core_boundary * scale[0], core_boundary * scale[0]], [0, xy_max[1]], color='red', linewidth=2,
                 linestyle='--', label='Threshold boundary')
    plt.legend(loc='lower right')
    _axis_labels(plt, title)
    plt.savefig(out_prefix + ".png")
    plt.close()


def log_likelihood(X, weights, means, covars, scale):
    """PopPUNK/bgmm.py:100-176 on the host: (logprob [n], lpr [n, K]) of the mixture at X / scale, through the lower
    Cholesky factor of each covariance (of cv + 1e-7 I where cv itself has none)."""
    Xs = np.asarray(X, dtype=np.float64) / np.asarray(scale, dtype=np.float64)
    means, covars = np.asarray(means, dtype=np.float64), np.asarray(covars, dtype=np.float64)
    lpr = np.empty((Xs.shape[0], len(means)), dtype=np.float64)
    for c, (mu, cv) in enumerate(zip(means, covars)):
        try:
            L = np.linalg.cholesky(cv)
        except np.linalg.LinAlgError:
            L = np.linalg.cholesky(cv + 1e-7 * np.eye(2))
        sol = np.linalg.solve(L, (Xs - mu).T).T
        lpr[:, c] = -0.5 * (np.sum(sol ** 2, axis=1) + 2 * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L))))
    lpr += np.log(np.asarray(weights, dtype=np.float64))
    top = lpr.max(axis=1)
    return top + np.log(np.exp(lpr - top[:, None]).sum(axis=1)), lpr


def contour_surfaces(model, assignments):
    """plot_contours' two surfaces on get_grid(0, 1, 100) (plot.py:395-404): (xx, yy, z, z_ll) with z the within-strain
    minus the between-strain responsibility from `model.assign(xy, values=True)` and z_ll the mixture's log
    likelihood, both in the reference's orientation.  As in the reference, `assign` divides the grid by the model's
    scale while the likelihood is taken at the grid itself."""
    from .bgmm import between_from_counts, within_from_counts
    xx, yy, xy = get_grid(0, 1, KDE_RESOLUTION)
    counts = _label_counts(assignments, 0, len(model.means))
    z = np.asarray(model.assign(xy.astype(np.float32), values=True), dtype=np.float64)
    z_diff = z[:, within_from_counts(model.means, counts, 0)] - z[:, between_from_counts(counts)]
    z_ll, _ = log_likelihood(xy, model.weights, model.means, model.covariances, np.array([1, 1]))
    return xx, yy, z_diff.reshape(xx.shape).T, z_ll.reshape(xx.shape).T


def plot_contours(model, assignments, title, out_prefix):
    """plot.py:375-414: the mixture's likelihood surface and, in red, its within / between decision boundary, written
    to <out_prefix>.pdf."""
    mpl, plt = _pyplot()
    xx, yy, z, z_ll = contour_surfaces(model, assignments)
    plt.figure(figsize=FIGSIZE, dpi=DPI, facecolor='w', edgecolor='k')
    plt.contour(xx, yy, z_ll, levels=np.linspace(z_ll.min(), z_ll.max(), 25))
    plt.contour(xx, yy, z, levels=[0], colors='r', linewidths=3)
    plt.title(title)
    plt.xlabel('Scaled core distance')
    plt.ylabel('Scaled accessory distance')
    plt.savefig(out_prefix + ".pdf")
    plt.close()


def distHistogram(dists, rank, outPrefix):
    """plot.py:443-466: the histogram of the nearest-neighbour distances kept at `rank`, written to
    <outPrefix>_rank_<rank>_histogram.png."""
    mpl, plt = _pyplot()
    plt.figure(figsize=FIGSIZE, dpi=DPI, facecolor='w', edgecolor='k')
    plt.hist(_host(dists), 50, facecolor='b', alpha=0.75)
    plt.title('Included nearest neighbour distances for rank ' + str(rank))
    plt.xlabel('Distance')
    plt.ylabel('Density')
    plt.grid(True)
    plt.savefig(outPrefix + "_rank_" + str(rank) + "_histogram.png")
    plt.close()
