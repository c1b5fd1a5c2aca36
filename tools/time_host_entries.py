"""Wall time of one multi-device host call on resident handles, one build of libppk_hip.so against another: the
dense, edge-list and neighbour-list entry points of ppk_host.hip at the sizes PopPUNK runs them, and a 130-genome
call that is all per-call overhead.

    python tools/time_host_entries.py --a OLD/libppk_hip.so --b poppunk_amd/csrc/libppk_hip.so --out result.json

Fresh child processes alternate the two libraries (PPK_LIBRARY), `--procs` of each; a child warms every call up, takes
the median of its repeats under a host clock (the calls are blocking: they end with the result in a host array) and a
digest of every result.  Per figure: the median of the per-process medians of each build, the range of A's (its own
run-to-run spread), and whether B's median lies inside that range.  The digests of A and B must agree.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import numpy as np
    import torch
    from poppunk_amd import _lib, engine, synth

    K = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    T = np.ascontiguousarray(synth.random_match_table(K), dtype=np.float32)
    kp, tp = K.ctypes.data_as(C.POINTER(C.c_int32)), T.ctypes.data_as(C.POINTER(C.c_float))
    llp, fp = C.POINTER(C.c_longlong), C.POINTER(C.c_float)
    lib = _lib.lib()
    sk = synth.make_sketches_device(11000, K, device="cuda:0")
    ref, qry, small = (engine.SketchDB(sk[:10000].contiguous(), 16, 14), engine.SketchDB(sk[10000:].contiguous(), 16, 14),
                       engine.SketchDB(sk[:130].contiguous(), 16, 14))
    sub = engine.SketchDB(sk[:2000].contiguous(), 16, 14)
    d, _ = engine.dist(sub, None, K, T)
    d = synth.tensor_to_numpy(d)
    x_max, y_max = synth.boundary_for_quantile(d, 0.02)
    inside = float(np.quantile(d[:, 0] / x_max + d[:, 1] / y_max, 0.02))      # the slope-2 line with 2 % of these pairs inside
    x_max, y_max = x_max * inside, y_max * inside
    sub.close()
    del d, sk
    torch.cuda.synchronize()
    flags = _lib.FLAG_RANDOM_CORRECT

    def handles(db, entries):
        return (C.c_void_p * entries)(*[db._h.value] * entries)

    def dense(r, q, entries=1):
        rows = r.n * q.n if q is not None else r.n * (r.n - 1) // 2
        rh, qh = handles(r, entries), handles(q, entries) if q is not None else None

        def call():
            out = np.empty((rows, 2), dtype=np.float32)          # a fresh pageable array, as PopPUNK's caller has
            t0 = time.perf_counter()
            rc = lib.ppk_query_dbs(rh, qh, entries, kp, tp, 1, flags, C.c_void_p(out.ctypes.data), None)
            dt = time.perf_counter() - t0
            _lib.check(rc, "ppk_query_dbs")
            return dt, (out,)
        return call

    def edges(entries):
        cap = 4 << 20                                             # 2 % of 5e7 pairs is 1e6 edges
        rh = handles(ref, entries)

        def call():
            out = np.empty((cap, 2), dtype=np.int64)
            n = C.c_size_t(0)
            t0 = time.perf_counter()
            rc = lib.ppk_query_edges_dbs(rh, None, entries, kp, tp, 1, flags, 2, x_max, y_max, 1.0, 1.0, 1,
                                         out.ctypes.data_as(llp), cap, C.byref(n), None)
            dt = time.perf_counter() - t0
            _lib.check(rc, "ppk_query_edges_dbs")
            return dt, (out[:n.value],)
        return call

    def knn(entries):
        m = ref.n * 6
        rh = handles(ref, entries)

        def call():
            oi, oj, od = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.float32)
            t0 = time.perf_counter()
            rc = lib.ppk_query_knn_dbs(rh, entries, kp, tp, 1, flags, 6, 0, oi.ctypes.data_as(llp), oj.ctypes.data_as(llp),
                                       od.ctypes.data_as(fp))
            dt = time.perf_counter() - t0
            _lib.check(rc, "ppk_query_knn_dbs")
            return dt, (oi, oj, od)
        return call

    figures = [("query_dbs 1000 x 10000", dense(ref, qry), 30), ("query_dbs 10000 self", dense(ref, None), 12),
               ("query_edges_dbs 10000 self (0,)", edges(1), 20), ("query_edges_dbs 10000 self (0,0)", edges(2), 20),
               ("query_knn_dbs 10000 self knn 6 (0,)", knn(1), 12), ("query_knn_dbs 10000 self knn 6 (0,0)", knn(2), 12),
               ("query_dbs 130 self", dense(small, None), 300)]
    res = {"source_hash": _lib.source_hash(), "figures": {}}
    for name, call, reps in figures:
        for _ in range(3):
            _, outs = call()
        digest = hashlib.sha1()
        for a in outs:
            digest.update(np.ascontiguousarray(a).tobytes())
        ts = sorted(call()[0] * 1e3 for _ in range(reps))
        res["figures"][name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "reps": reps, "rows": int(len(outs[0])),
                                "sha1": digest.hexdigest()}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="library A (the older build)")
    ap.add_argument("--b", help="library B")
    ap.add_argument("--procs", type=int, default=6, help="fresh processes per build")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-timeout", type=float, default=180.0)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    runs = {"a": [], "b": []}
    for i in range(args.procs):
        for side in ("a", "b") if i % 2 == 0 else ("b", "a"):
            env = dict(os.environ, PPK_LIBRARY=os.path.abspath(getattr(args, side)))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                               text=True, timeout=args.child_timeout)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("child with library %s failed (%d): no further process is started" % (side, p.returncode))
            runs[side].append(json.loads(line[0][7:]))
            report(args, runs)


def report(args, runs):
    out = {"a": args.a, "b": args.b, "processes": {s: len(r) for s, r in runs.items()},
           "source_hash": {s: r[0]["source_hash"] for s, r in runs.items() if r}, "figures": {}}
    if runs["a"] and runs["b"]:
        for name in runs["a"][0]["figures"]:
            med = {s: [r["figures"][name]["median_ms"] for r in runs[s]] for s in runs}
            sha = {r["figures"][name]["sha1"] for s in runs for r in runs[s]}
            out["figures"][name] = {
                "a_median_ms": statistics.median(med["a"]), "b_median_ms": statistics.median(med["b"]),
                "a_range_ms": [min(med["a"]), max(med["a"])], "b_range_ms": [min(med["b"]), max(med["b"])],
                "b_inside_a_range": min(med["a"]) <= statistics.median(med["b"]) <= max(med["a"]),
                "rows": runs["a"][0]["figures"][name]["rows"], "same_bits": len(sha) == 1,
                "a_process_medians_ms": med["a"], "b_process_medians_ms": med["b"]}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if len(runs["a"]) == len(runs["b"]) == args.procs:
        print(text)


if __name__ == "__main__":
    main()
