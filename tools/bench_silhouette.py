"""Silhouette on the MI355X (ppk_silhouette_dev): bench.py's 10 000-genome matrix and the 40 levels of
the sweep tools/bench_clusters.py uses.

    timeout -k 10 900 python tools/bench_silhouette.py [--out profiles/silhouette/bench_silhouette.json]

Records, HIP-event ms per call (median of --steps after four warm-ups; every call holds its own read-back):
  one_level / forty_levels   the call with one level (the sweep's middle one) and with all 40, rotating through four
              copies of the 400 MB matrix (cold Infinity Cache) and on one copy (hot), with the library's stage split;
              beside it, in the same run, a pure read of the same copies (torch.sum) and the ratio to it
  scratch_mb  the 40-level call under silhouette_scratch_mb = 64 / 256 / 1024, the three settings taken in turn,
              three rounds (the median of the rounds' medians is the figure)
  sklearn     if sklearn imports: silhouette_samples(metric='precomputed') on the float64 square of one level, on this
              host (the square's construction timed apart), and the largest |s - sklearn|
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
    from poppunk_amd import _lib, engine, synth
    lib = _lib.lib()
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n = a.samples
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    # the entry point takes distances in [0, 1]
    clamped = dist.clamp(0.0, 1.0)
    outside = int((clamped != dist).any(dim=1).sum().item())
    dist = clamped.contiguous()
    del clamped
    # bench.py f_rows_leg: the scaled matrix, 40 offsets from the 1 % to the 30 % quantile point, slope 2
    scale = dist.amax(dim=0)
    xs = (dist / scale).contiguous()
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0)
    m1 = np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    del xs
    levels_t, counts = engine.cluster_sweep_dev(i, j, o, n, 40)
    del i, j, o
    one_t = levels_t[20:21].contiguous()
    res = {"version": lib.ppk_version().decode(), "samples": n, "rows": int(dist.shape[0]), "levels": 40,
           "rows_clamped_to_0_1": outside, "steps": a.steps, "metric": "euclidean",
           "shift": engine.silhouette_shift(n), "clusters_per_level": counts.cpu().numpy().tolist(),
           "silhouette_scratch_mb_default": _lib.get_option("silhouette_scratch_mb")}

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
    for name, lv in (("one_level", one_t), ("forty_levels", levels_t)):
        call = lambda m, lv=lv: engine.silhouette_dev(m, lv)
        res[name] = {"cold": timed(call, lambda k: (mats[k % 4],)), "hot": timed(call, lambda k: (mats[0],)),
                     "stages_ms_per_call_cold": stages(lambda k, call=call: call(mats[k % 4]))}
        print(name, res[name], flush=True)
    res["pure_read_cold"] = timed(lambda m: torch.sum(m), lambda k: (mats[k % 4],))
    res["pure_read_hot"] = timed(lambda m: torch.sum(m), lambda k: (mats[0],))
    for name in ("one_level", "forty_levels"):
        res[name]["over_pure_read_cold"] = round(res[name]["cold"]["median_ms"] / res["pure_read_cold"]["median_ms"], 2)
    print({k: v for k, v in res.items() if k.startswith("pure")}, flush=True)

    # -- the cap on the band scratch: the three settings in turn, three rounds
    before = _lib.get_option("silhouette_scratch_mb")
    rounds = {mb: [] for mb in (64, 256, 1024)}
    try:
        for _ in range(3):
            for mb in rounds:
                _lib.set_option("silhouette_scratch_mb", mb)
                rounds[mb].append(timed(lambda m: engine.silhouette_dev(m, levels_t), lambda k: (mats[k % 4],))["median_ms"])
    finally:
        _lib.set_option("silhouette_scratch_mb", before)
    res["scratch_mb"] = {str(mb): {"rounds_median_ms": v, "median_ms": sorted(v)[1],
                                   "bands": -(-n // max(1, min(n, (mb << 20) // 5 * 4 // (((n + 3) & ~3) * 4))))}
                         for mb, v in rounds.items()}
    print("scratch_mb", res["scratch_mb"], flush=True)
    del mats[1:]

    s_t, n_labels, valid = engine.silhouette_dev(dist, levels_t)
    s = s_t.cpu().numpy()
    res["valid_levels"] = int(valid.sum().item())
    res["mean_silhouette_per_level"] = [None if np.isnan(v) else round(float(v), 6) for v in s.mean(axis=1)]

    # -- sklearn on this host, one level
    if a.no_sklearn:
        res["sklearn"] = "not run (--no-sklearn)"
    else:
        try:
            import sklearn
            from sklearn.metrics import silhouette_samples
        except ImportError:
            res["sklearn"] = "sklearn is not importable on this machine: not measured"
        else:
            x = dist.cpu().numpy()
            labels = one_t.cpu().numpy()[0]
            t0 = time.perf_counter()
            d = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
            sq = np.zeros((n, n), dtype=np.float64)
            sq[np.triu_indices(n, 1)] = d
            sq += sq.T
            t1 = time.perf_counter()
            want = silhouette_samples(sq, labels, metric="precomputed")
            t2 = time.perf_counter()
            res["sklearn"] = {"version": sklearn.__version__, "level": 20, "labels": int(len(np.unique(labels))),
                              "square_from_long_numpy_seconds": round(t1 - t0, 3),
                              "silhouette_samples_host_seconds": round(t2 - t1, 3),
                              "cpus": len(os.sched_getaffinity(0)),
                              "max_abs_difference": float(np.abs(s[20] - want).max())}
            print("sklearn", res["sklearn"], flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
