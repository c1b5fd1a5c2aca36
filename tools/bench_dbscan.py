"""Fitting and assigning the DBSCAN (HDBSCAN) model on the MI355X (ppk_dbscan_*), on the distance
matrix of bench.py's 10 000-genome self job (49 995 000 rows):

  fit      a seeded 100 000-row subsample (DBSCANModel.subsample_index, --seed), scaled as ClusterFit.fit does, at the
           first (min_samples, min_cluster_size) of DBSCANFit.fit's loop: core distances and spanning tree (HIP events
           and wall, median of --steps after one warm-up) and the host hierarchy (wall)
  assign   every row of the matrix through the fitted model, in calls of --chunk rows (HIP events per call, summed),
           with the grid search and the number of rows that fell back to a scan of everything (ppk_dbscan_stats);
           then the first --scan-rows rows again with option dbscan_search = 1, the plain scan: the yardstick, and the
           check that both give the same labels
  context  sklearn's HDBSCAN.fit on the same subsample on this host (--sklearn-n points of it; 0 = skip), and the
           numpy restatement of the assignment (tests/test_dbscan_host.py) on --restate-rows rows: the only CPU
           yardstick for the assignment here, the hdbscan package being absent

    timeout -k 10 1100 python tools/bench_dbscan.py [--out profiles/dbscan/bench_dbscan.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, steps):
    """(median HIP-event ms, median wall ms, last result) of fn() after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ev, wall, out = [], [], None
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(np.median(wall)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--prop", type=float, default=0.01, help="min_cluster_prop")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4 << 20)
    ap.add_argument("--assign-rows", type=int, default=0, help="rows to assign (0 = all)")
    ap.add_argument("--scan-rows", type=int, default=4 << 20)
    ap.add_argument("--sklearn-n", type=int, default=20000)
    ap.add_argument("--restate-rows", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from poppunk_amd import _lib, dbscan, engine, synth
    from poppunk_amd.models import DBSCANModel
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    db = engine.SketchDB(synth.make_sketches_device(args.genomes, kmers, device="cuda:0"), 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    n_rows = dist_t.shape[0]
    res = {"build": _lib.source_hash(), "genomes": args.genomes, "rows": n_rows, "seed": args.seed,
           "threads": len(os.sched_getaffinity(0))}

    idx = DBSCANModel.subsample_index(n_rows, args.max_samples, args.seed)
    sub_t = dist_t.clone() if idx is None else dist_t[torch.as_tensor(idx, device=dist_t.device)]
    scale_t = sub_t.amax(dim=0)
    sub_t = (sub_t / scale_t).contiguous()
    n = sub_t.shape[0]
    m, c = dbscan.min_samples_for(n, args.prop), dbscan.min_cluster_size_for(n)
    res["fit"] = {"n": n, "min_samples": m, "min_cluster_size": c}
    ev, wall, core2_t = timed(torch, lambda: engine.dbscan_core_dev(sub_t, m), args.steps)
    res["fit"]["core"] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3),
                          "d2_per_s": round(32.0 * n * n / (ev * 1e-3), 0)}
    ev, wall, mst = timed(torch, lambda: engine.dbscan_mst_dev(sub_t, core2_t), args.steps)
    res["fit"]["mst"] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3)}
    a, b, w = (x.cpu().numpy() for x in mst)
    t0 = time.perf_counter()
    tree = dbscan.fit_tree(a, b, w, n, c)
    res["fit"]["hierarchy_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["fit"]["clusters"] = tree.n_clusters
    res["fit"]["noise"] = int((tree.labels == -1).sum())
    res["fit"]["condensed_clusters"] = int(tree.cl_parent.shape[0])
    print(json.dumps(res["fit"]), flush=True)

    # the whole model fit as a user calls it (loop, subsample assignment, within / between labels)
    model = DBSCANModel()
    t0 = time.perf_counter()
    try:
        model.fit_dev(dist_t, max_num_clusters=100, min_cluster_prop=args.prop, max_samples=args.max_samples,
                      seed=args.seed, assign_points=False)
        res["model_fit"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "min_samples": model.min_samples,
                            "min_cluster_size": model.min_cluster_size, "n_clusters": model.n_clusters,
                            "within": model.within_label, "between": model.between_label}
    except RuntimeError as e:
        res["model_fit"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "error": str(e)}
        model._set_state(sub_t.cpu().numpy(), core2_t.cpu().numpy(), tree, m, c)
        model.scale, model.within_label, model.n_clusters, model.fitted = scale_t.cpu().numpy(), 0, tree.n_clusters, True
    print(json.dumps(res["model_fit"]), flush=True)

    import ctypes as C

    def assign_rows(rows, keep):
        total_ev, t0, counts, kept = 0.0, time.perf_counter(), {}, []
        for r0 in range(0, rows, args.chunk):
            r1 = min(rows, r0 + args.chunk)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lab = model.assign_dev(dist_t[r0:r1])
            e1.record()
            torch.cuda.synchronize()
            total_ev += e0.elapsed_time(e1)
            lab = lab.cpu().numpy()
            if r0 < keep:
                kept.append(lab[:keep - r0])
            for k, v in zip(*np.unique(lab, return_counts=True)):
                counts[int(k)] = counts.get(int(k), 0) + int(v)
            print("assigned %d of %d rows, %.1f s" % (r1, rows, total_ev * 1e-3), flush=True)
        return total_ev, (time.perf_counter() - t0) * 1e3, counts, np.concatenate(kept) if kept else None

    def scanned():
        v = C.c_ulonglong(0)
        _lib.check(_lib.lib().ppk_dbscan_stats(model.handle(0), C.byref(v)), "ppk_dbscan_stats")
        return int(v.value)

    rows = n_rows if args.assign_rows <= 0 else min(n_rows, args.assign_rows)
    scan_rows = min(rows, args.scan_rows)
    n_train, ms = model.points.shape[0], model.min_samples
    model.assign_dev(dist_t[:1024])                    # warm-up: the handle's upload and the first launch
    torch.cuda.synchronize()
    before = scanned()
    ev, wall, counts, first = assign_rows(rows, scan_rows)
    res["assign"] = {"rows": rows, "training_points": n_train, "min_samples": ms, "search": "grid",
                     "event_ms": round(ev, 1), "wall_ms": round(wall, 1), "rows_per_s": round(rows / (ev * 1e-3), 0),
                     "rows_scanned_in_full": scanned() - before, "label_counts": counts}
    print(json.dumps(res["assign"]), flush=True)
    if scan_rows > 0:
        _lib.set_option("dbscan_search", 1)
        ev, wall, _, again = assign_rows(scan_rows, scan_rows)
        _lib.set_option("dbscan_search", 0)
        res["assign_scan"] = {"rows": scan_rows, "search": "scan", "event_ms": round(ev, 1), "wall_ms": round(wall, 1),
                              "rows_per_s": round(scan_rows / (ev * 1e-3), 0),
                              "d2_per_s": round(34.0 * scan_rows * n_train / (ev * 1e-3), 0),
                              "equal_to_grid": bool(np.array_equal(first, again))}
        print(json.dumps(res["assign_scan"]), flush=True)

    if args.restate_rows > 0:
        import test_dbscan_host as H
        X = dist_t[:args.restate_rows].cpu().numpy()
        t0 = time.perf_counter()
        want = H.ref_assign(H.scale_rows(X, model.scale), model.points, model.core2, ms, model, block=64)
        dt = time.perf_counter() - t0
        got = model.assign_dev(dist_t[:args.restate_rows]).cpu().numpy()
        res["restatement"] = {"what": "numpy restatement of the assignment, one process", "rows": args.restate_rows,
                              "wall_s": round(dt, 2), "rows_per_s": round(args.restate_rows / dt, 1),
                              "equal_to_device": bool(np.array_equal(got, want))}
        print(json.dumps(res["restatement"]), flush=True)
    if args.sklearn_n > 0:
        try:
            from sklearn.cluster import HDBSCAN
            k = min(args.sklearn_n, n)
            P = sub_t[:k].cpu().numpy().astype(np.float64)
            mk, ck = dbscan.min_samples_for(k, args.prop), dbscan.min_cluster_size_for(k)
            t0 = time.perf_counter()
            sk = HDBSCAN(min_samples=mk + 1, min_cluster_size=ck, algorithm="kd_tree").fit(P)
            res["sklearn"] = {"n": k, "min_samples": mk, "min_cluster_size": ck,
                              "fit_wall_s": round(time.perf_counter() - t0, 2),
                              "clusters": int(sk.labels_.max()) + 1, "threads": res["threads"]}
        except ImportError:
            res["sklearn"] = {"error": "sklearn is not installed"}
        print(json.dumps(res["sklearn"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
