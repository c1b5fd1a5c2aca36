"""Fitting the BGMM on the MI355X (ppk_bgmm_fit*), on the distance matrix of bench.py's 10 000-genome
self job (49 995 000 rows):

  subsample  PopPUNK's shape: a seeded 100 000-row subsample (DBSCANModel.subsample_index, --seed), K = 2 and 4, n_init =
             5 with the own initialisation: wall time of BGMMModel.fit_dev (assign_points=False), the iterations and
             k-means passes it made, and the split of one iteration: the pass (ppk_bgmm_stats_dev, HIP events, median of
             --steps after a warm-up), the host M-step (ppk_bgmm_mstep, wall, median of 200 calls), and what is left of
             fit wall / passes (launches, the read-back and its synchronisation, Python)
  k16        the pass alone at K = 16 on the subsample (four sweeps of the rows inside one launch), from the state of a
             one-run fit: what the components beyond the fourth cost
  whole      every row of the matrix (max_samples=None), K = 4: the pass by HIP events, and the whole fit (wall)
  sklearn    BayesianGaussianMixture with fit2dMultiGaussian's settings on the same subsample (float32, as PopPUNK
             passes it) on this host, --sklearn 1 (0 = skip); threadpoolctl is not assumed: the threads are what the
             environment gives numpy's BLAS

    timeout -k 10 1100 python tools/bench_bgmm_fit.py [--out profiles/bgmm_fit/bench_bgmm_fit.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pass_ms(torch, fn, steps):
    fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    return float(np.median(ev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sklearn", type=int, default=1)
    ap.add_argument("--whole-k", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from poppunk_amd import _lib, engine, synth
    from poppunk_amd.models import BGMMModel, DBSCANModel
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    db = engine.SketchDB(synth.make_sketches_device(args.genomes, kmers, device="cuda:0"), 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    n_rows = dist_t.shape[0]
    res = {"build": _lib.source_hash(), "genomes": args.genomes, "rows": n_rows, "seed": args.seed,
           "threads": len(os.sched_getaffinity(0)), "subsample": {}, "whole": {}}

    def mstep_us(model):
        st = model.fit_result.state
        params = engine.bgmm_fit_params(st.K)
        sums = np.ones((st.K, 7))
        sums[:, 1:3] = 0.0
        sums[:, 6] = -0.1
        piv, w0, out, lb = np.zeros((st.K, 2)), np.eye(2).ravel().copy(), _lib.BgmmState(), C.c_double()
        f64p = C.POINTER(C.c_double)
        t0 = time.perf_counter()
        for _ in range(200):
            _lib.lib().ppk_bgmm_mstep(C.byref(params), sums.ctypes.data_as(f64p), piv.ctypes.data_as(f64p),
                                      w0.ctypes.data_as(f64p), C.byref(out), C.byref(lb))
        return (time.perf_counter() - t0) / 200 * 1e6

    def one(K, max_samples):
        BGMMModel.fit_dev(dist_t, K, max_samples=max_samples, seed=args.seed, assign_points=False, n_init=1)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = BGMMModel.fit_dev(dist_t, K, max_samples=max_samples, seed=args.seed, assign_points=False)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        r = m.fit_result
        idx = None if max_samples is None else DBSCANModel.subsample_index(n_rows, max_samples, args.seed)
        idx_t = None if idx is None else torch.as_tensor(idx, device=dist_t.device)
        ev = pass_ms(torch, lambda: engine.bgmm_stats_dev(dist_t, r.state, m.scale, index_t=idx_t), args.steps)
        # every pass of the fit: 3 for the rows' check and the covariance prior, per run the k-means passes, 2 for the
        # initial statistics and one per iteration
        passes = 3 + int(r.kmeans_iter.sum()) + 2 * len(r.init_n_iter) + int(r.init_n_iter.sum())
        ms = mstep_us(m)
        return {"K": K, "n_train": r.n_train, "n_init": len(r.init_n_iter), "fit_wall_ms": round(wall, 2),
                "best_init": r.best_init, "n_iter": r.n_iter, "converged": r.converged, "lower_bound": r.lower_bound,
                "iterations_all_runs": int(r.init_n_iter.sum()), "kmeans_passes_all_runs": int(r.kmeans_iter.sum()),
                "passes": passes, "pass_event_ms": round(ev, 4), "mstep_host_us": round(ms, 2),
                "wall_per_pass_ms": round(wall / passes, 4),
                "rest_per_pass_ms": round(wall / passes - ev - ms * 1e-3, 4),
                "pass_bytes_per_s": round((16 if idx is not None else 8) * r.n_train / (ev * 1e-3), 0),
                "weights": [round(float(w), 6) for w in m.weights], "within": m.within_label, "between": m.between_label}

    for K in (2, 4):
        res["subsample"]["K%d" % K] = one(K, args.max_samples)
        print(json.dumps(res["subsample"]["K%d" % K]), flush=True)
    m16 = BGMMModel.fit_dev(dist_t, 16, max_samples=args.max_samples, seed=args.seed, assign_points=False, n_init=1)
    idx_t = torch.as_tensor(DBSCANModel.subsample_index(n_rows, args.max_samples, args.seed), device=dist_t.device)
    res["k16"] = {"K": 16, "n_train": m16.fit_result.n_train, "pass_event_ms": round(pass_ms(
        torch, lambda: engine.bgmm_stats_dev(dist_t, m16.fit_result.state, m16.scale, index_t=idx_t), args.steps), 4)}
    print(json.dumps(res["k16"]), flush=True)
    res["whole"]["K%d" % args.whole_k] = one(args.whole_k, None)
    print(json.dumps(res["whole"]), flush=True)

    if args.sklearn:
        try:
            from sklearn.mixture import BayesianGaussianMixture
            idx = DBSCANModel.subsample_index(n_rows, args.max_samples, args.seed)
            sub = dist_t[torch.as_tensor(idx, device=dist_t.device)].cpu().numpy()
            sub = sub / np.amax(sub, axis=0)
            res["sklearn"] = {}
            for K in (2, 4):
                np.random.seed(1)
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sk = BayesianGaussianMixture(n_components=K, n_init=5, covariance_type="full",
                                                 weight_concentration_prior=0.1, mean_precision_prior=0.1,
                                                 mean_prior=np.array([0, 0])).fit(sub)
                res["sklearn"]["K%d" % K] = {"fit_wall_s": round(time.perf_counter() - t0, 2), "n_iter": int(sk.n_iter_),
                                             "converged": bool(sk.converged_), "dtype": str(sub.dtype),
                                             "threads": res["threads"]}
                print(json.dumps(res["sklearn"]), flush=True)
        except ImportError:
            res["sklearn"] = {"error": "sklearn is not installed"}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
