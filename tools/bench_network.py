"""Network sweep on the MI355X (ppk_network_sweep_dev): bench.py's 10 000-genome matrix and its 40-offset
thresholdIterate1D sweep, scored on the device.

    timeout -k 10 900 python tools/bench_network.py [--out profiles/network/bench_network.json]

Records: HIP-event ms and wall ms per call (median of --steps after two warm-ups; the sweep's triples are resident),
the library's stage split (validate / csr / components / wedges / triangles), the counts, and a CPU restatement of the
same counts with scipy / numpy (NOT graph-tool, which is not in this image) for the final graph on 16 threads.
--pmc-only: only the network calls (five), the program a counter pass (rocprofv3 --pmc) runs."""
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
        out[name] = {"ms": round(float(ms), 5), "count": int(cnt)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--pmc-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, synth
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(10_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    # bench.py f_rows_leg: the scaled matrix, 40 offsets from the 1 % to the 30 % quantile point, slope 2
    scale = dist.amax(dim=0)
    xs = (dist / scale).contiguous()
    del dist
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0)
    m1 = np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    n = 10_000
    m = int(i.shape[0])

    def call():
        return engine.network_sweep_dev(i, j, o, n, 40)

    if a.pmc_only:
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        print("pmc-only: 5 calls, %d edges" % m)
        return
    res = {"version": lib.ppk_version().decode(), "samples": n, "offsets": 40, "edges": m, "steps": a.steps}
    for _ in range(2):
        stats, _ = call()
    torch.cuda.synchronize()
    wall, evs = [], []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        evs.append(e0.elapsed_time(e1))
    res["event_ms"] = round(float(np.median(evs)), 4)
    res["wall_ms"] = round(float(np.median(wall)), 4)
    lib.ppk_prof_stages_enable(1)
    stage_table(lib)
    for _ in range(a.steps):
        call()
    torch.cuda.synchronize()
    lib.ppk_prof_stages_enable(0)
    st = stage_table(lib)
    res["stages_ms_per_call"] = {k: round(v["ms"] / max(v["count"], 1), 4) for k, v in st.items()}
    s = stats.cpu().numpy()
    res["final_counts"] = {"edges": int(s[-1, 0]), "components": int(s[-1, 1]), "triangles": int(s[-1, 2]),
                           "triples": int(s[-1, 3])}
    res["offsets_with_edges"] = int((np.diff(np.concatenate(([0], s[:, 0]))) > 0).sum())
    # work of the triangle stage: sum over oriented edges (u, v) of |N+(v)|, the LDS lookups it makes
    ih, jh = i.cpu().numpy(), j.cpu().numpy()
    lo, hi = np.minimum(ih, jh), np.maximum(ih, jh)
    outdeg = np.bincount(lo, minlength=n)
    res["triangle_lookups"] = int(outdeg[hi].sum())
    if not a.no_cpu:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        t0 = time.perf_counter()
        A = coo_matrix((np.ones(m, dtype=np.float32), (lo, hi)), shape=(n, n)).tocsr()
        A = (A + A.T).tocsr()
        nc, _ = connected_components(A, directed=False)
        D = A.toarray()
        T = int(round(float(((D @ D) * D).sum(dtype=np.float64)) / 6))
        deg = np.asarray(A.sum(1)).ravel().astype(np.int64)
        W = int((deg * (deg - 1) // 2).sum())
        cpu_s = time.perf_counter() - t0
        res["cpu_restatement"] = {
            "what": "scipy connected_components + dense float32 numpy A@A (triangles) of the FINAL graph only; "
                    "scipy/numpy, not graph-tool",
            "threads": os.environ.get("OMP_NUM_THREADS"), "seconds_one_graph": round(cpu_s, 3),
            "seconds_for_all_offsets_estimate": round(cpu_s * res["offsets_with_edges"], 2),
            "agrees": [nc, T, W] == [int(s[-1, 1]), int(s[-1, 2]), int(s[-1, 3])]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
