"""Neighbour-joining trees on the MI355X (ppk_nj_dev), on the core distances of bench.py's synthetic
10 000-genome matrix: the first n = 1 000, 4 000 and 10 000 samples, as the resident long form (one column of the
[n_pairs, 2] matrix, read in place) and as its squared form.

    timeout -k 10 900 python tools/bench_nj.py [--out profiles/nj/bench_nj.json]

Records per (n, form): HIP-event ms and wall ms per call (median of --steps after two warm-ups; inputs resident), the
library's stage split (load / rowsum / scan / update / compact / tail), the bytes the scan launches read (from the
host's copy of the schedule: every join outside the tail reads its whole triangle of m slots once) over the scan
time, and that both forms give the same bits.  CPU baseline: the numpy restatement of the same rule
(tests/test_nj_host.py) on n = 1 000 and 2 000 with 16 threads allowed; larger n are extrapolated as n^3."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAIL_R = 256          # ppk_nj.hip kTailR


def stage_table(lib):
    import ctypes as C
    buf = C.create_string_buffer(1 << 16)
    lib.ppk_prof_stages_read(buf, len(buf), 1)
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, cnt = line.split("\t")
        out[name] = {"ms": round(float(ms), 5), "count": int(cnt)}
    return out


def scan_bytes(n):
    """Bytes the scan launches read: the float64 triangle of the current m slots, once per join outside the tail."""
    total, m = 0, n
    for r in range(n, TAIL_R, -1):
        if 8 * (m - r) >= m:
            m = r
        total += m * (m - 1) // 2 * 8
    return total


def measure(lib, call, steps):
    import torch
    for _ in range(2):
        out = call()
    torch.cuda.synchronize()
    wall, evs = [], []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        evs.append(e0.elapsed_time(e1))
    lib.ppk_prof_stages_enable(1)
    stage_table(lib)
    call()
    torch.cuda.synchronize()
    lib.ppk_prof_stages_enable(0)
    st = stage_table(lib)
    return out, {"event_ms": round(float(np.median(evs)), 3), "wall_ms": round(float(np.median(wall)), 3),
                 "stages_ms_one_profiled_call": {k: v["ms"] for k, v in st.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, synth
    lib = _lib.lib()
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    res = {"version": lib.ppk_version().decode(), "steps": a.steps, "runs": []}

    sk, _ = synth.make_sketches(10_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    for n in [int(x) for x in a.sizes.split(",")]:
        long_t = dist if n == 10_000 else engine.prune_long_dev(dist, 10_000, np.arange(n))
        sq = engine.long_to_square_dev(long_t, 0, n)
        outs = {}
        for form, src in (("long", long_t), ("square", sq)):
            kw = {"col": 0} if form == "long" else {}
            out, rec = measure(lib, lambda: engine.nj_dev(src, n=n, **kw), a.steps)
            outs[form] = out
            st = rec["stages_ms_one_profiled_call"]
            b = scan_bytes(n)
            rec.update(n=n, form=form, scan_bytes=b,
                       scan_TB_per_s=round(b / (st.get("scan", 0.0) * 1e-3) / 1e12, 3) if st.get("scan") else None)
            res["runs"].append(rec)
            print(json.dumps(rec), flush=True)
        res["runs"][-1]["same_bits_as_long"] = bool(torch.equal(outs["long"][0], outs["square"][0]) and torch.equal(
            outs["long"][1].view(torch.int64), outs["square"][1].view(torch.int64)))
        del long_t, sq
    if not a.no_cpu:
        from test_nj_host import nj_same_rule
        sq = engine.long_to_square_dev(engine.prune_long_dev(dist, 10_000, np.arange(2000)), 0, 2000).cpu().numpy()
        cpu = {}
        for n in (1000, 2000):
            t0 = time.perf_counter()
            nj_same_rule(sq[:n, :n])
            cpu[str(n)] = round(time.perf_counter() - t0, 2)
        cpu["10000_extrapolated_n3"] = round(cpu["2000"] * 125, 0)
        res["cpu_numpy_restatement_s"] = cpu
        print(json.dumps(cpu), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
