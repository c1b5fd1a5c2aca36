"""Cluster numbers and pair sums on the MI355X (ppk_cluster_sweep_dev, ppk_cluster_pair_sums_dev):
bench.py's 10 000-genome matrix and its 40-offset thresholdIterate1D sweep.

    timeout -k 10 900 python tools/bench_clusters.py [--out profiles/clusters/bench_clusters.json]

Records, HIP-event ms per call (median of --steps after four warm-ups; every call ends with its own read-back):
  sweep       the cluster numbers of all 40 graphs (the sweep's triples are resident), with the library's stage split
  pair_sums   the one pass over the matrix with those 40 levels, rotating through four copies of the 400 MB matrix
              (cold Infinity Cache) and on one copy (hot); beside it, in the same run, a pure read of the same copies
              (torch.sum, which reads 8 B per row and writes nothing to speak of) and kernel 2's assignThreshold
  reference_route   what scripts/poppunk_iterate.py does, on this device: one engine.dist per cluster of the family
              (the cluster's sketches as a database of their own), largest clusters first, until the family is done
              or --route-seconds have passed (checked after every cluster); the family step on the host is timed apart
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
    ap.add_argument("--route-seconds", type=float, default=120.0)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, iterate, synth
    lib = _lib.lib()
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n = 10_000
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    # bench.py f_rows_leg: the scaled matrix, 40 offsets from the 1 % to the 30 % quantile point, slope 2
    scale = dist.amax(dim=0)
    xs = (dist / scale).contiguous()
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0)
    m1 = np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    del xs
    res = {"version": lib.ppk_version().decode(), "samples": n, "rows": int(dist.shape[0]), "offsets": 40,
           "edges": int(i.shape[0]), "steps": a.steps}

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

    # -- the 40-level sweep labels
    sweep = lambda: engine.cluster_sweep_dev(i, j, o, n, 40)
    res["sweep"] = timed(sweep, lambda k: ())
    lib.ppk_prof_stages_enable(1)
    stage_table(lib)
    for _ in range(a.steps):
        sweep()
    torch.cuda.synchronize()
    lib.ppk_prof_stages_enable(0)
    res["sweep"]["stages_ms_per_call"] = {k: round(v["ms"] / a.steps, 4) for k, v in stage_table(lib).items()}
    levels_t, counts = sweep()
    res["clusters_per_level"] = counts.cpu().numpy().tolist()
    print("sweep", res["sweep"], flush=True)

    # -- the pair-sum pass against a pure read of the same matrix
    mats = [dist] + [dist.clone() for _ in range(3)]
    res["pair_sums_cold"] = timed(lambda m: engine.cluster_pair_sums_dev(m, levels_t), lambda k: (mats[k % 4],))
    res["pair_sums_hot"] = timed(lambda m: engine.cluster_pair_sums_dev(m, levels_t), lambda k: (mats[0],))
    res["pure_read_cold"] = timed(lambda m: torch.sum(m), lambda k: (mats[k % 4],))
    res["pure_read_hot"] = timed(lambda m: torch.sum(m), lambda k: (mats[0],))
    out = torch.empty(dist.shape[0], dtype=torch.float32, device=dist.device)
    res["assign_threshold_cold"] = timed(lambda m: engine.assign_threshold_dev(m, 2, 0.01, 0.1, out=out),
                                         lambda k: (mats[k % 4],))
    res["pair_sums_over_pure_read"] = round(res["pair_sums_cold"]["median_ms"] / res["pure_read_cold"]["median_ms"], 2)
    res["pair_sums_GBs"] = round(8.0 * dist.shape[0] / res["pair_sums_cold"]["median_ms"] / 1e6, 1)
    lib.ppk_prof_stages_enable(1)
    stage_table(lib)
    for k in range(a.steps):
        engine.cluster_pair_sums_dev(mats[k % 4], levels_t)
    torch.cuda.synchronize()
    lib.ppk_prof_stages_enable(0)
    res["pair_sums_stages_ms_per_call"] = {k: round(v["ms"] / a.steps, 4) for k, v in stage_table(lib).items()}
    del mats
    print({k: v for k, v in res.items() if k.startswith(("pair", "pure", "assign"))}, flush=True)

    # -- the whole iterate step, and the reference's route on this device
    levels = levels_t.cpu().numpy()
    names = ["g%d" % k for k in range(n)]
    t0 = time.perf_counter()
    family, where, order, _ = iterate.family_of_levels(levels, names)
    res["family"] = {"clusters": len(family), "host_seconds": round(time.perf_counter() - t0, 3)}
    print("family", res["family"], flush=True)
    t0 = time.perf_counter()
    s, c, shift = engine.cluster_pair_sums_dev(dist, levels_t)
    means = iterate.cluster_means(levels, s.cpu().numpy(), c.cpu().numpy(), shift)
    res["one_pass_all_means_seconds"] = round(time.perf_counter() - t0, 4)
    # (rows of a sweep are numbered 1 .. K already, so `where`'s cluster numbers index `means` as they stand)
    assert np.array_equal(iterate.dense_levels(levels), levels)
    index = {name: v for v, name in enumerate(names)}
    done, pairs, worst = 0, 0, 0.0
    t0 = time.perf_counter()
    for cluster in order:
        members = np.array(sorted(index[x] for x in family[cluster]), dtype=np.int64)
        sub = engine.SketchDB(np.ascontiguousarray(sk[members]), 16, 14, device=0)
        d, _ = engine.dist(sub, None, kmers, tbl)
        pi = float(d[:, 0].mean().item())
        sub.close()
        t, cnum = where[cluster]
        worst = max(worst, abs(pi - float(means[t, cnum])))
        done += 1
        pairs += int(d.shape[0])
        if time.perf_counter() - t0 > a.route_seconds:
            break
        if done % 100 == 0:
            print("route", done, round(time.perf_counter() - t0, 1), flush=True)
    seconds = time.perf_counter() - t0
    res["reference_route"] = {"clusters_done": done, "of": len(family), "seconds": round(seconds, 3),
                              "pairs_computed": pairs, "rows_of_the_matrix": int(dist.shape[0]),
                              "seconds_whole_family_estimate": round(seconds * len(family) / done, 1),
                              "max_abs_mean_difference": worst,
                              "what": "per cluster, largest first: SketchDB of its sketches + engine.dist + the "
                                      "float32 mean of column 0; the estimate scales by cluster count"}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
