#!/usr/bin/env python3
"""Generates tests/golden/density.npz: what the reference's plot_scatter hands matplotlib, for small matrices.

Run in the BUILD container only (needs the reference checkout, numpy and scikit-learn); what it writes is data (input
matrices, the arrays passed to plt.contour and plt.scatter, seeds, error figures) and is committed, the reference is not.

Reference code executed (pulled out of its module with `ast`, as make_golden_network.py does, and run unmodified but
for the one constant noted below):
  PopPUNK/plot.py    plot_scatter, get_grid
under the real numpy / sklearn.utils.shuffle / sklearn.neighbors.KernelDensity of this image, with a recording stand-in
for `plt` and a `random` whose randint returns the case's seed.

Cases (keys <case>_*):
  blobs3000   3 000 rows: a within-strain blob near the origin and a between-strain blob
  blobs500    500 rows of the same kind
  sample1500  1 500 rows through the seeded sample route: the constant max_plot_samples = 1000000 of plot_scatter is
              replaced by 1000 in the syntax tree (nothing else changes), so utils.shuffle draws 1 000 rows
Per case: x (the float32 [n, 2] input), seed, max_plot_samples, contour_x, contour_y, z, levels (the four arguments of
plt.contour: xx * scale[0], yy * scale[1], z, levels[1:]), scatter_x, scatter_y (the two arguments of plt.scatter),
scale, savefig (the file name relative to out_prefix), title, xlabel, ylabel, and e_ref = max |z - z_direct| / max z,
where z_direct is a float64 numpy sum of the same kernel over the same scaled float32 rows: sklearn's own rounding
(its log-sum-exp over tree nodes), the reference side's error that the tests' tolerance is built from.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_network as mgn          # noqa: E402

REF = mgn.REF


class RecordingPlt:
    """The part of matplotlib.pyplot plot_scatter calls; keeps every call's arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args, **kwargs):
            self.calls.append((name, args, kwargs))
        return record

    def one(self, name):
        hits = [c for c in self.calls if c[0] == name]
        assert len(hits) == 1, (name, len(hits))
        return hits[0]


class FixedRandom:
    def __init__(self, seed):
        self.seed = seed

    def randint(self, lo, hi):
        assert lo <= self.seed <= hi
        return self.seed


def reference_namespace(plt, seed, max_plot_samples):
    from sklearn import utils
    from sklearn.neighbors import KernelDensity
    ns = {"np": np, "os": os, "plt": plt, "utils": utils, "KernelDensity": KernelDensity, "random": FixedRandom(seed)}
    path = os.path.join(REF, "PopPUNK", "plot.py")
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("plot_scatter", "get_grid"):
            if node.name == "plot_scatter" and max_plot_samples != 1000000:
                hits = [c for c in ast.walk(node) if isinstance(c, ast.Constant) and c.value == 1000000]
                assert len(hits) == 1
                hits[0].value = max_plot_samples
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    assert "plot_scatter" in ns and "get_grid" in ns
    return ns


def blobs(n, seed):
    """A within-strain blob near the origin (a fifth of the rows) and a between-strain blob, float32, shuffled."""
    rng = np.random.RandomState(seed)
    nw = n // 5
    within = np.abs(np.column_stack([rng.normal(0.002, 0.001, nw), rng.normal(0.02, 0.012, nw)]))
    between = np.abs(np.column_stack([rng.normal(0.02, 0.004, n - nw), rng.normal(0.3, 0.05, n - nw)]))
    x = np.vstack([within, between]).astype(np.float32)
    return x[rng.permutation(n)]


def z_direct(xs, h=0.03):
    """The float64 sum of the Epanechnikov kernel on the reference's grid, in its orientation."""
    g = np.linspace(0, 1, 100)
    p = xs.astype(np.float64)
    s = np.zeros((100, 100))
    for lo in range(0, len(p), 500):
        q = p[lo:lo + 500]
        d2 = ((q[:, 0, None] - g[None, :]) ** 2)[:, :, None] + ((q[:, 1, None] - g[None, :]) ** 2)[:, None, :]
        s += np.maximum(1.0 - d2 / (h * h), 0.0).sum(axis=0)
    # s is [core node, accessory node]; z.reshape(xx.shape).T is [accessory node, core node]
    return s.T * 2.0 / (np.pi * h * h * len(p))


def run_case(name, x, seed, max_plot_samples, out):
    plt = RecordingPlt()
    ns = reference_namespace(plt, seed, max_plot_samples)
    work = x.copy()                      # (plot_scatter divides its argument in place unless it sampled)
    ns["plot_scatter"](work, "out_dir", "Distances of " + name)
    _, cargs, ckw = plt.one("contour")
    _, sargs, skw = plt.one("scatter")
    assert skw == {"s": 1, "alpha": 1} and ckw["cmap"] == "plasma"
    z = np.asarray(cargs[2])
    sx, sy = np.asarray(sargs[0]), np.asarray(sargs[1])
    assert sx.dtype == np.float32 and len(sx) == min(len(x), max_plot_samples)
    # the scaled rows the reference fitted: its scatter arguments are xs * scale
    if len(x) > max_plot_samples:
        from sklearn import utils
        rows = utils.shuffle(x, random_state=seed)[0:max_plot_samples, ]
    else:
        rows = x
    scale = np.amax(rows, axis=0)
    xs = rows / scale
    assert np.array_equal(xs[:, 0] * scale[0], sx) and np.array_equal(xs[:, 1] * scale[1], sy)
    zd = z_direct(xs)
    e_ref = float(np.abs(z - zd).max() / z.max())
    print("%-11s rows %5d  fitted %5d  max z %.4g  e_ref %.3g" % (name, len(x), len(rows), z.max(), e_ref))
    out.update({
        name + "_x": x, name + "_seed": np.int64(seed), name + "_max_plot_samples": np.int64(max_plot_samples),
        name + "_contour_x": np.asarray(cargs[0]), name + "_contour_y": np.asarray(cargs[1]), name + "_z": z,
        name + "_levels": np.asarray(ckw["levels"]), name + "_scatter_x": sx, name + "_scatter_y": sy,
        name + "_scale": scale, name + "_e_ref": np.float64(e_ref),
        name + "_savefig": np.array(os.path.relpath(plt.one("savefig")[1][0], "out_dir")),
        name + "_title": np.array(plt.one("title")[1][0]), name + "_xlabel": np.array(plt.one("xlabel")[1][0]),
        name + "_ylabel": np.array(plt.one("ylabel")[1][0]),
    })


def main():
    out = {}
    run_case("blobs3000", blobs(3000, 11), 1234, 1000000, out)
    run_case("blobs500", blobs(500, 12), 77, 1000000, out)
    run_case("sample1500", blobs(1500, 13), 4321, 1000, out)
    path = os.path.join(HERE, "density.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
