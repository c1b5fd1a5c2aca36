"""Density grids on the MI355X (ppk_density_kde_dev, ppk_density_counts_dev) on bench.py's
10 000-genome matrix (49 995 000 rows).

    timeout -k 10 900 python tools/bench_density.py [--out profiles/density/bench_density.json]

Records, HIP-event ms per call (median of --steps after four warm-ups; every call ends with its own read-back), cold
(four copies of the 400 MB matrix in rotation, so the Infinity Cache holds none of it) and warm (one copy):
  kde_all       the Epanechnikov sums of every row on plot_scatter's 100 x 100 grid, h = 0.03, the scale taken on the
                device (stages: scale, kde), and with the scale passed in
  kde_index     the same over a 1 000 000-entry index list (the rows sklearn.utils.shuffle would keep)
  counts        the 1760 x 1280 occupancy raster without labels and with a BGMM fit's labels, with option
                density_hot_table 1 and 0 (the contention experiment of the counts pass), on the matrix as it is and
                with every row crowded into a fiftieth of each axis (warm); kde_crowded: the sums of those rows
  kde_presum    the kde pass (scale passed in, warm) with option density_kde_presum 0, 4, 16, 32 and 64 (the contention
                experiment of the kde pass), on the matrix as it is and on the crowded rows
  pure_read     torch.sum of the same copies, re-measured in this run: what reading the matrix costs
  sklearn       KernelDensity.fit + score_samples of the 1 000 000-row sample on this machine's host (wall seconds),
                or why it was not measured
No threshold is asserted here: the numbers are the record."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=10_000)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, models, plot, synth
    lib = _lib.lib()
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n = a.samples
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    rows = int(dist.shape[0])
    res = {"version": lib.ppk_version().decode(), "samples": n, "rows": rows, "steps": a.steps,
           "grid": "100 x 100, h = 0.03", "raster": "1760 x 1280"}

    def timed(fn, args_of):
        for k in range(4):
            fn(*args_of(k))
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for k, (e0, e1) in enumerate(ev):
            e0.record()
            fn(*args_of(k))
            e1.record()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return {"median_ms": round(t[len(t) // 2], 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5)}

    def stages(fn):
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        for k in range(a.steps):
            fn(k)
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        return {k: round(v["ms"] / a.steps, 4) for k, v in stage_table(lib).items()}

    mats = [dist] + [dist.clone() for _ in range(3)]
    cold, warm = (lambda k: (mats[k % 4],)), (lambda k: (mats[0],))
    g = np.linspace(0, 1, plot.KDE_RESOLUTION)
    h = plot.KDE_BANDWIDTH
    scale = dist.amax(dim=0).cpu().numpy()

    res["pure_read_cold"] = timed(lambda m: torch.sum(m), cold)
    res["pure_read_warm"] = timed(lambda m: torch.sum(m), warm)

    kde = lambda m: engine.density_kde_dev(m, g, g, h)                     # noqa: E731
    kde_scaled = lambda m: engine.density_kde_dev(m, g, g, h, scale=scale)      # noqa: E731
    res["kde_all_cold"] = timed(kde, cold)
    res["kde_all_warm"] = timed(kde, warm)
    res["kde_all_scale_given_cold"] = timed(kde_scaled, cold)
    res["kde_all_stages_ms_per_call"] = stages(lambda k: kde(mats[k % 4]))
    res["kde_all_over_pure_read"] = round(res["kde_all_cold"]["median_ms"] / res["pure_read_cold"]["median_ms"], 2)
    sums, shift, _ = kde(dist)
    res["kde_shift"] = shift
    top = np.sort(sums.cpu().numpy().ravel().astype(np.float64))[::-1]
    res["kde_share_of_the_sum_in_the_10_heaviest_cells"] = round(float(top[:10].sum() / max(top.sum(), 1.0)), 4)
    print({k: v for k, v in res.items() if k.startswith(("kde", "pure"))}, flush=True)

    idx = plot.shuffle_indices(rows, 1234, 1_000_000)
    idx_t = torch.as_tensor(idx, dtype=torch.int64, device=dist.device)
    kde_idx = lambda m: engine.density_kde_dev(m, g, g, h, idx_t=idx_t)     # noqa: E731
    res["kde_index_cold"] = timed(kde_idx, cold)
    res["kde_index_warm"] = timed(kde_idx, warm)
    res["kde_index_stages_ms_per_call"] = stages(lambda k: kde_idx(mats[k % 4]))
    print({k: v for k, v in res.items() if k.startswith("kde_index")}, flush=True)

    # -- the occupancy raster, with and without a BGMM fit's labels, through the hot-pixel table and without it
    t0 = time.perf_counter()
    model = models.BGMMModel.fit_dev(dist, 2, max_samples=100000, seed=42)
    labels = model.assign_dev(dist)
    res["bgmm_fit_and_assign_seconds"] = round(time.perf_counter() - t0, 3)
    raster, _ = plot.raster_for(scale)
    old = _lib.get_option("density_hot_table")
    old_presum = _lib.get_option("density_kde_presum")
    try:
        for table in (1, 0):
            _lib.set_option("density_hot_table", table)
            tag = "counts_table_%d" % table
            plain = lambda m: engine.density_counts_dev(m, raster)                      # noqa: E731
            lab = lambda m: engine.density_counts_dev(m, raster, labels, 0, 2)          # noqa: E731
            res[tag + "_cold"] = timed(plain, cold)
            res[tag + "_warm"] = timed(plain, warm)
            res[tag + "_labels_cold"] = timed(lab, cold)
            res[tag + "_labels_warm"] = timed(lab, warm)
        # the same pass with the rows crowded into a fiftieth of each axis (some 900 pixels): what contention costs
        crowded = (dist * 0.02).contiguous()
        for table in (1, 0):
            _lib.set_option("density_hot_table", table)
            res["counts_crowded_table_%d" % table] = timed(lambda m: engine.density_counts_dev(m, raster), lambda k: (crowded,))
        res["kde_crowded"] = timed(lambda m: engine.density_kde_dev(m, g, g, h, scale=scale), lambda k: (crowded,))
        # the contention experiment of the kde pass: lanes of a wave that share a window summed before the LDS add, for
        # groups of at least so many lanes (0: off), on the matrix as it is and on the crowded rows; the same sums
        res["kde_presum_default"] = old_presum
        want = [engine.density_kde_dev(m, g, g, h, scale=scale)[0] for m in (dist, crowded)]
        for group in (0, 4, 16, 32, 64):
            _lib.set_option("density_kde_presum", group)
            res["kde_presum_%d" % group] = timed(kde_scaled, warm)
            res["kde_crowded_presum_%d" % group] = timed(kde_scaled, lambda k: (crowded,))
            assert all(torch.equal(engine.density_kde_dev(m, g, g, h, scale=scale)[0], w)
                       for m, w in zip((dist, crowded), want))
        del crowded
    finally:
        _lib.set_option("density_hot_table", old)
        _lib.set_option("density_kde_presum", old_presum)
    counts, outside = engine.density_counts_dev(dist, raster)
    c = counts.cpu().numpy().ravel()
    res["counts_outside"] = int(outside.cpu()[0])
    res["counts_pixels_occupied"] = int((c > 0).sum())
    res["counts_share_of_the_rows_in_the_1024_fullest_pixels"] = round(float(np.sort(c)[::-1][:1024].sum() / max(rows, 1)), 4)
    res["counts_over_pure_read"] = round(res["counts_table_%d_cold" % old]["median_ms"] / res["pure_read_cold"]["median_ms"], 2)
    print({k: v for k, v in res.items() if k.startswith("counts")}, flush=True)

    # -- the reference's route on this host: the 1 000 000-row sample through sklearn
    if a.no_sklearn:
        res["sklearn"] = {"measured": False, "why": "--no-sklearn"}
    else:
        try:
            from sklearn.neighbors import KernelDensity
            x = dist[idx_t].cpu().numpy()
            x = x / np.amax(x, axis=0)
            _, _, xy = plot.get_grid(0, 1, plot.KDE_RESOLUTION)
            t0 = time.perf_counter()
            est = KernelDensity(bandwidth=h, metric='euclidean', kernel='epanechnikov', algorithm='ball_tree').fit(x)
            t1 = time.perf_counter()
            z = np.exp(est.score_samples(xy))
            t2 = time.perf_counter()
            s, sh, nr = engine.density_kde_dev(dist, g, g, h, idx_t=idx_t)
            zd = plot.kde_values(s.cpu().numpy(), sh, h, nr)
            import sklearn
            res["sklearn"] = {"measured": True, "version": sklearn.__version__, "rows": int(len(x)),
                              "fit_seconds": round(t1 - t0, 3), "score_seconds": round(t2 - t1, 3),
                              "max_abs_difference_over_max_z": float(np.abs(zd - z.reshape(100, 100).T).max() / z.max())}
        except ImportError as e:
            res["sklearn"] = {"measured": False, "why": "scikit-learn is not importable here: %s" % e}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
