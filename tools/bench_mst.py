"""Minimum spanning forests on the MI355X (ppk_mst_dev), on two graphs:
  (a) the final graph of bench.py's 40-offset sweep of 10 000 genomes (built as tools/bench_network.py builds it),
      weighted by core distance (ppk_edge_weights_dev);
  (b) the 10-nearest-neighbour lists of 100 000 synthetic genomes (engine.knn_from_sketches), weighted by distance.

    timeout -k 10 900 python tools/bench_mst.py [--out profiles/mst/bench_mst.json]

Records per graph: HIP-event ms and wall ms per call (median of --steps after two warm-ups; inputs resident), the
library's stage split (validate / rank / boruvka / labels / compact), the Boruvka rounds that hooked (counted on the
host by the same algorithm on the same ranks: they depend only on the graph and the order), and scipy's
minimum_spanning_tree on the same edges on this host (strictly positive weights: csgraph drops explicit zeros), with
the check that the sorted tree weights are equal."""
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


def boruvka_rounds(e, w, n):
    """Hooking rounds of Boruvka on ranks (w, min, max, index): the rounds the device runs before its early exit."""
    lo, hi = e.min(axis=1), e.max(axis=1)
    order = np.lexsort((np.arange(len(e)), hi, lo, w.astype(np.float64) + 0.0))
    u, v = lo[order], hi[order]
    comp = np.arange(n)
    rounds = 0
    while True:
        cu, cv = comp[u], comp[v]
        cross = np.flatnonzero(cu != cv)
        if cross.size == 0:
            return rounds
        rounds += 1
        best = np.full(n, len(e), dtype=np.int64)
        np.minimum.at(best, cu[cross], cross)
        np.minimum.at(best, cv[cross], cross)
        roots = np.flatnonzero(best < len(e))
        parent = comp.copy()
        for r in roots.tolist():
            b = best[r]
            other = cv[b] if cu[b] == r else cu[b]
            if not (best[other] == b and r < other):
                parent[r] = other
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        comp = parent[comp]


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
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    lib.ppk_prof_stages_enable(0)
    st = stage_table(lib)
    return out, {"event_ms": round(float(np.median(evs)), 4), "wall_ms": round(float(np.median(wall)), 4),
                 "stages_ms_per_call": {k: round(v["ms"] / max(v["count"], 1), 4) for k, v in st.items()}}


def graph_record(lib, e_t, w_t, n, steps, cpu):
    from poppunk_amd import engine
    (tree, comps, _), res = measure(lib, lambda: engine.mst_dev(e_t, w_t, n), steps)
    e, w = e_t.cpu().numpy(), w_t.cpu().numpy()
    res.update(vertices=n, edges=int(e.shape[0]), tree_edges=int(tree.numel()), components=int(comps),
               boruvka_rounds=boruvka_rounds(e, w, n))
    if cpu:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
        t0 = time.perf_counter()
        csr = coo_matrix((w.astype(np.float64), (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
        t1 = time.perf_counter()
        t = minimum_spanning_tree(csr)
        t2 = time.perf_counter()
        res["scipy_ms"] = {"to_csr": round((t1 - t0) * 1e3, 2), "minimum_spanning_tree": round((t2 - t1) * 1e3, 2)}
        res["scipy_tree_weights_equal"] = bool(np.array_equal(np.sort(t.data),
                                                              np.sort(w[tree.cpu().numpy()].astype(np.float64))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, synth
    lib = _lib.lib()
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    res = {"version": lib.ppk_version().decode(), "steps": a.steps}

    # (a) bench.py's sweep graph, core distance
    sk, _ = synth.make_sketches(10_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    xs = (dist / dist.amax(dim=0)).contiguous()
    sample = xs[::20].cpu().numpy()
    m0, m1 = np.quantile(sample, 0.01, axis=0), np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, _ = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    e_t = torch.stack([i, j], dim=1).contiguous()
    _, wres = measure(lib, lambda: engine.edge_weights_dev(dist, e_t, "core"), a.steps)
    w_t = engine.edge_weights_dev(dist, e_t, "core")
    zero = int((w_t <= 0).sum())
    keep = w_t > 0
    res["sweep_graph"] = graph_record(lib, e_t[keep].contiguous(), w_t[keep].contiguous(), 10_000, a.steps,
                                      not a.no_cpu)
    res["sweep_graph"]["zero_weight_edges_dropped"] = zero
    res["sweep_graph"]["edge_weights"] = wres
    del dist, xs

    # (b) 10-NN lists of 100 000 genomes
    sk, _ = synth.make_sketches(100_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    gi, gj, gd = engine.knn_from_sketches(db, kmers, tbl, 10)
    db.close()
    keep = gd > 0
    res["knn_graph"] = graph_record(lib, torch.stack([gi[keep], gj[keep]], dim=1).contiguous(),
                                    gd[keep].to(torch.float32).contiguous(), 100_000, a.steps, not a.no_cpu)
    res["knn_graph"]["zero_weight_edges_dropped"] = int((~keep).sum())
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
