"""Fitting the refine boundary on the MI355X (refine.refineFit, ppk_refine_score_dev, ppk_refine_local_*; DESIGN.md
3.14), on the scaled distance matrix of bench.py's 10 000-genome self job (49 995 000 rows) and the line of its sweep
leg (the 1 % to the 30 % quantile point, slope 2).

    timeout -k 10 900 python tools/bench_refine_fit.py [--out profiles/refine_fit/bench_refine_fit.json]

Records
  fit        refineFit's wall time with option refine_local = 1 and = 0, split into the global sweep, the creation of
             the bracket handle and the evaluations of the local search (wall, around the scorer's calls), the number
             of evaluations scipy made, the bounds and the result -- which must not depend on the option
  split      base / candidate / never rows of the bracket
  stages     the library's stage table (ppk_prof_stage names) summed over one fit of each kind
  per_eval   at every position the local search evaluated: HIP-event ms of the bracket handle's evaluation, of
             ppk_refine_score_dev, and of the full path with the entry points the parent commit already had
             (edge_threshold_dev + network_sweep_dev at one offset), medians of --steps; the three give the same counts
When the global minimum sits at an end of the sweep (no local step), the bracket around the clamped minimum is timed
at five positions inside it instead, and `local_step` says so."""
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


class Timed:
    """refine.DeviceScorer with wall clocks around its calls"""

    def __init__(self, scorer, torch):
        self.s, self.torch, self.n_rows = scorer, torch, scorer.n_rows
        self.ms = {"sweep": 0.0, "create": 0.0, "evaluations": 0.0}
        self.split = None

    def _clock(self, key, fn):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        self.torch.cuda.synchronize()
        self.ms[key] += (time.perf_counter() - t0) * 1e3
        return out

    def sweep_1d(self, *a):
        return self._clock("sweep", lambda: self.s.sweep_1d(*a))

    def sweep_2d(self, *a):
        return self._clock("sweep", lambda: self.s.sweep_2d(*a))

    def score(self, *a):
        return self._clock("evaluations", lambda: self.s.score(*a))

    def bracket(self, *a):
        h = self._clock("create", lambda: self.s.bracket(*a))
        if h is None:
            return None
        self.split = h.split
        outer = self

        class Handle:
            split = h.split

            def eval(self, x, y):
                return outer._clock("evaluations", lambda: h.eval(x, y))

            def close(self):
                h.close()
        return Handle()


def event_ms(torch, fn, steps):
    fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--genomes", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, refine, synth
    lib = _lib.lib()
    n = a.genomes
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    scale = dist.amax(dim=0)
    xs = (dist / scale).contiguous()
    del dist
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0).astype(np.float64)
    m1 = np.quantile(sample, 0.30, axis=0).astype(np.float64)
    names = [str(k) for k in range(n)]
    one = np.array([1.0, 1.0])
    res = {"version": lib.ppk_version().decode(), "samples": n, "rows": int(xs.shape[0]), "steps": a.steps,
           "mean0": m0.tolist(), "mean1": m1.tolist(), "fit": {}}
    old = _lib.get_option("refine_local")
    infos = {}
    try:
        for local in (1, 0, 1, 0):          # the first pair warms every allocation up; the second is recorded
            _lib.set_option("refine_local", local)
            scorer = Timed(refine.DeviceScorer(xs), torch)
            lib.ppk_prof_stages_enable(1)
            stage_table(lib)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = refine.refineFit(scorer, names, m0.copy(), m1.copy(), one, 0.0, 0.0)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            lib.ppk_prof_stages_enable(0)
            info = refine.last_fit
            infos[local] = info
            res["fit"]["refine_local_%d" % local] = {
                "wall_ms": round(wall, 3), "wall_split_ms": {k: round(v, 3) for k, v in scorer.ms.items()},
                "evaluations": len(info["evals"]), "local_path": info["local_path"], "bounds": info["bounds"],
                "result": [float(v) for v in out], "split_base_candidates_never": scorer.split,
                "stages": stage_table(lib)}
    finally:
        _lib.set_option("refine_local", old)
    f1, f0 = res["fit"]["refine_local_1"], res["fit"]["refine_local_0"]
    res["same_fit"] = f1["result"] == f0["result"] and [e[:2] for e in infos[1]["evals"]] == [e[:2] for e in infos[0]["evals"]]

    # per evaluation: the three ways to the same four counts
    g = (m1[1] - m0[1]) / (m1[0] - m0[0])
    info = infos[1]
    res["local_step"] = info["bounds"] is not None
    if info["bounds"] is not None:
        bounds, positions = info["bounds"], [e[0] for e in info["evals"]]
    else:
        s_range = np.linspace(0.0, float(np.hypot(*(m1 - m0))), 40)
        k = int(np.clip(np.argmin(info["global_s"]), 1, 38))
        bounds = [float(s_range[k - 1]), float(s_range[k + 1])]
        positions = np.linspace(bounds[0], bounds[1], 7)[1:-1].tolist()
    lo = [np.float32(v) for v in refine.boundary_of_s(bounds[0], m0, m1, g, 2)]
    hi = [np.float32(v) for v in refine.boundary_of_s(bounds[1], m0, m1, g, 2)]
    create_ms, handle = event_ms(torch, lambda: engine.RefineLocal.create(xs, 2, lo[0], lo[1], hi[0], hi[1]), 1)
    res["bracket"] = {"bounds": bounds, "lo": [float(v) for v in lo], "hi": [float(v) for v in hi],
                      "create_event_ms": round(create_ms, 3),
                      "split_base_candidates_never": handle.split if handle is not None else None}
    rows = []
    for s in positions:
        x, y = refine.boundary_of_s(s, m0, m1, g, 2)
        score_ms, st_score = event_ms(torch, lambda: engine.refine_score_dev(xs, 2, x, y), a.steps)
        full_ms, st_full = event_ms(
            torch, lambda: engine.network_stats_dev(engine.edge_threshold_dev(xs, 2, x, y), n)[0].cpu().numpy(), a.steps)
        row = {"s": float(s), "counts": [int(v) for v in st_score], "refine_score_ms": round(score_ms, 4),
               "full_path_ms": round(full_ms, 4), "agree": bool(np.array_equal(st_score, st_full))}
        if handle is not None:
            br_ms, st_br = event_ms(torch, lambda: handle.eval(x, y), a.steps)
            row["bracket_ms"] = round(br_ms, 4)
            row["agree"] = row["agree"] and bool(np.array_equal(st_score, st_br))
        rows.append(row)
    if handle is not None:
        handle.close()
    res["per_eval"] = rows
    for key in ("bracket_ms", "refine_score_ms", "full_path_ms"):
        vals = [r[key] for r in rows if key in r]
        if vals:
            res["median_" + key] = round(float(np.median(vals)), 4)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
