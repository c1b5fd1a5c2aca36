"""Embeddings on the MI355X (ppk_embed_weights_dev + ppk_embed_dev), from the device population
model's sketches (synth.make_sketches_device) through engine.knn_from_sketches(..., dist_col=1) to Y, at the
default settings (perplexity 20, maxIter 10^7, 65 536 workers, 5 repulsive samples).

    timeout -k 10 600 python tools/bench_embed.py [--out profiles/embed/bench_embed.json]

Records per n: end-to-end wall ms from resident sketches (neighbours + calibration + loop, synchronised), the HIP
event ms of the calibration and of the loop (median of --steps after one warm-up), the library's stage split
(check / calibrate / weights / init / step / apply) from one extra profiled call, and from the schedule: iterations,
launches, pair updates and int64 atomics per second of loop time.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (profiles/embed/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stage_table(lib):
    import ctypes as C
    buf = C.create_string_buffer(1 << 16)
    lib.ppk_prof_stages_read(buf, len(buf), 1)
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, cnt = line.split("\t")
        out[name] = {"ms": round(float(ms), 4), "count": int(cnt)}
    return out


def timed(call, steps):
    import torch
    call()
    torch.cuda.synchronize()
    evs = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        evs.append(e0.elapsed_time(e1))
    return round(float(np.median(evs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--knn", type=int, default=50)
    ap.add_argument("--max-iter", type=int, default=10 ** 7)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, mandrake, synth
    lib = _lib.lib()
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    res = {"version": lib.ppk_version().decode(), "steps": a.steps, "knn": a.knn, "max_iter": a.max_iter,
           "runs": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        db = engine.SketchDB(synth.make_sketches_device(n, kmers, seed=5), 16, 14, device=0)
        knn = min(a.knn, n - 1)
        mandrake.embed_sketches(db, kmers, tbl, 20.0, kNN=knn, maxIter=a.max_iter, seed=1)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mandrake.embed_sketches(db, kmers, tbl, 20.0, kNN=knn, maxIter=a.max_iter, seed=1).cpu()
        wall = (time.perf_counter() - t0) * 1e3
        i, j, d = engine.knn_from_sketches(db, kmers, tbl, knn, dist_col=1)
        db.close()
        P = engine.embed_weights_dev(i, j, d, n, 20.0)
        cal_ms = timed(lambda: engine.embed_weights_dev(i, j, d, n, 20.0), a.steps)
        loop_ms = timed(lambda: engine.embed_dev(i, j, P, n, 1, max_iter=a.max_iter), a.steps)
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        engine.embed_weights_dev(i, j, d, n, 20.0)
        engine.embed_dev(i, j, P, n, 1, max_iter=a.max_iter)
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        st = stage_table(lib)
        W = min(engine.EMBED_WORKERS, n)
        T = max(1, round(a.max_iter / W))
        pairs = T * W * 6                       # 1 attractive + 5 repulsive per worker (a few skipped k == l)
        atomics = pairs * 4 + T * ((W + 63) // 64) * 2
        rec = {"n": n, "knn": knn, "workers": W, "iterations": T, "launches": 2 * T + 4,
               "wall_ms_sketches_to_Y": round(wall, 2), "calibrate_event_ms": cal_ms, "loop_event_ms": loop_ms,
               "iterations_per_s": round(T / (loop_ms * 1e-3)), "launches_per_s": round((2 * T + 4) / (loop_ms * 1e-3)),
               "pair_updates_per_s": round(pairs / (loop_ms * 1e-3)),
               "int64_atomics_per_s": round(atomics / (loop_ms * 1e-3)),
               "stages_ms_one_profiled_call": {k: v["ms"] for k, v in st.items()}}
        res["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        del i, j, d, P
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
