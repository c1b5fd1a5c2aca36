"""BGMM assignment on the MI355X: kernel 2 on the resident 10 000-genome matrix (49 995 000 rows), the fused
sketches -> BGMM -> edge list path against the line-boundary one, and config 4's shape through the host call.

    timeout -k 10 900 python tools/bench_bgmm.py [--out profiles/bgmm/bench.json]

Methodology of bench.py's kernel2 leg: HIP events on the stream the launches go to, warm-up, median of repeats;
`cold` rotates through four distinct copies of the 400 MB matrix (no pass finds its input in the 256 MB Infinity
Cache).  Both fused paths are tuned to a similar edge fraction (the line through the 10 % quantile of the core
distance, the BGMM's within component on the same pairs)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-config4", action="store_true")
    ap.add_argument("--pmc-only", action="store_true",
                    help="only the kernel-2 assignment launches (assignThreshold, BGMM labels at K = 2 and 4), 5 each: "
                         "the program a counter pass (rocprofv3 --pmc) runs")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, synth
    from poppunk_amd.models import BGMMModel
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    res = {"version": lib.ppk_version().decode(), "steps": a.steps}
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(10_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    d10k, _ = engine.dist(db, None, kmers, tbl)
    torch.cuda.synchronize()
    n = d10k.shape[0]
    res["rows"] = n
    sample = d10k[:: max(1, n // 200_000)].cpu().numpy()
    scale = np.amax(sample, axis=0)
    xs = sample / scale
    q = float(np.quantile(xs[:, 0], 0.1))
    close = np.zeros(xs.shape[0], dtype=bool)
    close[np.argsort(xs[:, 0], kind="stable")[: xs.shape[0] // 10]] = True

    def model(K):
        mus = [xs[close].mean(0), xs[~close].mean(0)]
        covs = [np.cov(xs[close].T) + 1e-6 * np.eye(2), np.cov(xs[~close].T) + 1e-6 * np.eye(2)]
        w = [0.1, 0.9]
        for k in range(K - 2):
            mus.append(np.array([0.5 + 0.1 * k, 0.2]))
            covs.append(np.eye(2) * 0.01)
            w.append(0.01)
        return BGMMModel(np.array(w) / sum(w), np.array(mus), np.array(covs), scale, 0, 1)

    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    mats = [d10k] + [d10k.clone() for _ in range(3)]

    def timed(fn, rotate=True, steps=a.steps):
        for i in range(4):
            fn(mats[i % 4 if rotate else 0])
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for i, (s, e) in enumerate(ev):
            s.record()
            fn(mats[i % 4 if rotate else 0])
            e.record()
        torch.cuda.synchronize()
        t = sorted(s.elapsed_time(e) for s, e in ev)
        return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}

    labels = torch.empty(n, dtype=torch.int32, device=dev)
    if a.pmc_only:
        assign_out = torch.empty(n, dtype=torch.float32, device=dev)
        for _ in range(5):
            lib.ppk_assign_threshold_dev(C.c_void_p(d10k.data_ptr()), n, 2, 0.1, 0.1, C.c_void_p(assign_out.data_ptr()),
                                         stream)
        for K in (2, 4):
            mdl = model(K)
            for _ in range(5):
                lib.ppk_bgmm_assign_dev(C.c_void_p(d10k.data_ptr()), n, C.byref(mdl.model),
                                        C.c_void_p(labels.data_ptr()), None, stream)
        torch.cuda.synchronize()
        print("pmc-only done")
        return
    cap = 1 << 26
    edges = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    n_edges = torch.zeros(1, dtype=torch.int64, device=dev)
    assign_out = torch.empty(n, dtype=torch.float32, device=dev)
    x_max = float(np.quantile(sample[:, 0], 0.1)) * 2.0
    y_max = float(np.amax(sample[:, 1])) * 4.0
    k2 = {}
    k2["assign_threshold"] = timed(lambda m: lib.ppk_assign_threshold_dev(
        C.c_void_p(m.data_ptr()), n, 2, x_max, y_max, C.c_void_p(assign_out.data_ptr()), stream))
    for K in (2, 4):
        mdl = model(K)
        resp = torch.empty((n, K), dtype=torch.float32, device=dev)
        k2["assign_labels_K%d" % K] = timed(lambda m: lib.ppk_bgmm_assign_dev(
            C.c_void_p(m.data_ptr()), n, C.byref(mdl.model), C.c_void_p(labels.data_ptr()), None, stream))
        k2["assign_labels_resp_K%d" % K] = timed(lambda m: lib.ppk_bgmm_assign_dev(
            C.c_void_p(m.data_ptr()), n, C.byref(mdl.model), C.c_void_p(labels.data_ptr()),
            C.c_void_p(resp.data_ptr()), stream), steps=max(5, a.steps // 2))
        k2["edges_K%d" % K] = timed(lambda m: lib.ppk_bgmm_edges_dev(
            C.c_void_p(m.data_ptr()), n, 0, C.byref(mdl.model), 0, C.c_void_p(edges.data_ptr()), cap,
            C.c_void_p(n_edges.data_ptr()), stream))
        torch.cuda.synchronize()
        k2["edges_K%d_count" % K] = int(n_edges.item())
        del resp
    res["kernel2_10k"] = k2
    print(json.dumps({"kernel2_10k": k2}), flush=True)
    del mats
    torch.cuda.empty_cache()

    # fused: 10 000 genomes against themselves, line boundary vs BGMM, similar edge fractions
    fz = {}
    for name, fn in (
            ("line", lambda: engine.dist_edges(db, None, kmers, tbl, slope=0, x_max=q, y_max=0.0,
                                               scale=tuple(float(v) for v in scale), inclusive=False)),
            ("bgmm_K2", lambda mdl=model(2): engine.dist_bgmm_edges(db, None, kmers, tbl, model=mdl.model)),
            ("bgmm_K4", lambda mdl=model(4): engine.dist_bgmm_edges(db, None, kmers, tbl, model=mdl.model))):
        e, _ = fn()
        fz[name + "_edges"] = int(e.shape[0])
        ts = []
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        for _ in range(max(5, a.steps // 2)):
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            t.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(t))
        ts.sort()
        fz[name] = {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3)}
    fz["bgmm_K2_over_line"] = round(fz["bgmm_K2"]["median_ms"] / fz["line"]["median_ms"], 4)
    fz["bgmm_K4_over_line"] = round(fz["bgmm_K4"]["median_ms"] / fz["line"]["median_ms"], 4)
    res["fused_10k"] = fz
    print(json.dumps({"fused_10k": fz}), flush=True)
    db.close()

    if not a.skip_config4:
        # config 4: 50 000 queries x 10 000 references through the host call.  Queries and references are drawn from the
        # same clusters (one sample in six is a reference), and the models' within component is fitted to the low tail of
        # the query x reference distances, so the list holds a few percent of the pairs, as a real assignment's would.
        big, _ = synth.make_sketches(60_000, kmers, cluster_size=60, seed=11)
        is_ref = np.arange(60_000) % 6 == 0
        ref = engine.SketchDB(big[is_ref], 16, 14, device=0)
        qry = engine.SketchDB(big[~is_ref], 16, 14, device=0)
        qr, _ = engine.dist(ref, qry, kmers, tbl, q_begin=0, q_end=512)
        qs = qr.cpu().numpy()
        del qr
        c4_scale = np.amax(qs, axis=0)
        qxs = qs / c4_scale
        low = np.zeros(qxs.shape[0], dtype=bool)
        low[np.argsort(qxs[:, 0], kind="stable")[: qxs.shape[0] // 30]] = True       # ~3 % of the pairs

        def c4_model(K):
            mus = [qxs[low].mean(0), qxs[~low].mean(0)]
            covs = [np.cov(qxs[low].T) + 1e-6 * np.eye(2), np.cov(qxs[~low].T) + 1e-6 * np.eye(2)]
            w = [0.03, 0.97]
            for k in range(K - 2):
                mus.append(np.array([0.5 + 0.1 * k, 0.2]))
                covs.append(np.eye(2) * 0.01)
                w.append(0.01)
            return BGMMModel(np.array(w) / sum(w), np.array(mus), np.array(covs), c4_scale, 0, 1)

        c4_q = float(np.quantile(qxs[:, 0], 1 / 30))
        c4 = {}

        def host_timed(fn):
            fn()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                e, _ = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return {"median_ms": round(ts[1], 2), "edges": int(e.shape[0]), "edge_fraction": round(e.shape[0] / 5e8, 4)}
        for K in (2, 4):
            mdl = c4_model(K)
            c4["bgmm_K%d" % K] = host_timed(lambda: mdl.edges_host(ref, qry, kmers, tbl))
        c4["line"] = host_timed(lambda: engine.edges_host(ref, qry, kmers, tbl, slope=0, x_max=c4_q, y_max=0.0,
                                                          scale=tuple(float(v) for v in c4_scale), inclusive=False))
        res["config4_host"] = c4
        print(json.dumps({"config4_host": c4}), flush=True)
        ref.close()
        qry.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
