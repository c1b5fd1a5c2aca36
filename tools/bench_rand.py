"""Contingency sums on the MI355X (ppk_contingency_sums_dev): every level against every level of two
families of 40 clusterings.

    timeout -k 10 900 python tools/bench_rand.py [--out profiles/rand/bench_rand.json]

Records, HIP-event ms per call (median of --steps after two warm-ups; every call holds its own read-back):
  sweep_10k   the 40 levels of the sweep tools/bench_silhouette.py uses on bench.py's 10 000-genome matrix, all 780
              pairs (B = A), with the library's stage split
  synthetic_1m   40 levels of 1 000 000 samples: a nested family of 38 (every level merges the classes of the one
              before at random, 1 000 000 classes down to a handful) and two independent labelings (300 and 50 000
              labels), all 780 pairs, with the stage split
  beside each, in the same run: a pure read of the same label arrays on the device (torch.sum), and on this host
  sklearn.metrics.adjusted_rand_score over the same pairs -- all 780 at 10 000 samples; at 1 000 000 a stated sample of
  pairs, the total extrapolated from their mean and marked as such -- and whether the adjusted indices are the same
  floats
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


def sweep_levels(n):
    """tools/bench_silhouette.py's family: 40 boundaries from the 1 % to the 30 % quantile point, slope 2."""
    from poppunk_amd import engine, synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    xs = (dist / dist.amax(dim=0)).contiguous()
    del dist
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0)
    m1 = np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    del xs
    levels_t, counts = engine.cluster_sweep_dev(i, j, o, n, 40)
    return levels_t.contiguous(), counts.cpu().numpy().tolist()


def synthetic_levels(n, seed=1):
    """int32 [40, n]: 38 nested levels (level t + 1 maps the classes of level t onto 0.7 times as many, at random) and
    two independent labelings."""
    rng = np.random.default_rng(seed)
    levels = [np.arange(1, n + 1, dtype=np.int64)]
    k = n
    while len(levels) < 38:
        k_next = max(1, int(k * 0.7))
        onto = rng.integers(1, k_next + 1, k + 1)
        levels.append(onto[levels[-1]])
        k = k_next
    levels.append(rng.integers(1, 301, n))
    levels.append(rng.integers(1, 50001, n))
    return np.stack(levels).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10_000)
    ap.add_argument("--synthetic", type=int, default=1_000_000)
    ap.add_argument("--sklearn-pairs", type=int, default=12, help="pairs sklearn is timed on at the synthetic size")
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, scores
    lib = _lib.lib()
    res = {"version": lib.ppk_version().decode(), "steps": a.steps, "levels": 40, "pairs": 780,
           "options": {k: _lib.get_option(k) for k in ("rand_scratch_mb", "rand_batch", "rand_wave_max", "rand_window")},
           "cpus": len(os.sched_getaffinity(0))}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return {"median_ms": round(t[len(t) // 2], 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5)}

    def stages(fn):
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        return {k: round(v["ms"] / a.steps, 4) for k, v in stage_table(lib).items()}

    def sklearn_over(levels, pairs, total_pairs):
        if a.no_sklearn:
            return "not run (--no-sklearn)"
        try:
            import sklearn
            from sklearn.metrics import adjusted_rand_score
        except ImportError:
            return "sklearn is not importable on this machine: not measured"
        _, adjusted, _ = scores.rand_of_levels(levels_dev)
        same = True
        t0 = time.perf_counter()
        for x, y in pairs:
            same = (adjusted_rand_score(levels[x], levels[y]) == adjusted[x, y]) and same
        seconds = time.perf_counter() - t0
        out = {"version": sklearn.__version__, "pairs_timed": len(pairs), "seconds": round(seconds, 3),
               "seconds_per_pair": round(seconds / len(pairs), 5), "same_floats_as_the_device_call": bool(same)}
        if len(pairs) < total_pairs:
            out["pairs_sampled"] = [list(p) for p in pairs]
            out["seconds_all_pairs_EXTRAPOLATED"] = round(seconds / len(pairs) * total_pairs, 1)
        return out

    all_pairs = [(x, y) for x in range(40) for y in range(x + 1, 40)]
    for name in ("sweep_10k", "synthetic_1m"):
        if name == "sweep_10k":
            levels_dev, counts = sweep_levels(a.samples)
            levels = levels_dev.cpu().numpy()
            pairs = all_pairs
        else:
            levels = synthetic_levels(a.synthetic)
            levels_dev = torch.as_tensor(levels, device="cuda:0")
            counts = [int(len(np.unique(row))) for row in levels]
            rng = np.random.default_rng(2)
            pairs = [all_pairs[k] for k in sorted(rng.choice(len(all_pairs), a.sklearn_pairs, replace=False))]
        call = lambda: engine.contingency_sums_dev(levels_dev)
        r = {"samples": int(levels.shape[1]), "clusters_per_level": counts, "call": timed(call),
             "stages_ms_per_call": stages(call), "pure_read_of_the_labels": timed(lambda: torch.sum(levels_dev))}
        r["over_pure_read"] = round(r["call"]["median_ms"] / r["pure_read_of_the_labels"]["median_ms"], 1)
        r["sklearn_adjusted_rand_score_host"] = sklearn_over(levels, pairs, len(all_pairs))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del levels_dev
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
