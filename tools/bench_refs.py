"""Reference picking on the MI355X (ppk_pick_refs_dev) on two networks:

  bench10k   bench.py's 10 000-genome self job: its scaled distance matrix, refine.refineFit along the line from the
             1 % to the 30 % quantile point (tools/bench_refine_fit.py's fit), the edges within the fitted boundary
  config4    BASELINE config 4's shape as tools/bench_assign.py builds it: the first 10 000 of 60 000 genomes, the
             model's own self edges under a slope-2 boundary with 2 % of the query-reference pairs inside

Run from the repository root (it imports tools.bench_assign and tools.bench_network, as the neighbouring tools do):

    timeout -k 10 900 python tools/bench_refs.py [--out profiles/refs/bench_refs.json] [--dump DIR]
    python tools/bench_refs.py --stand-in DIR [--out FILE]      # no GPU: where the reference checkout is

Records per network, clique mode and fast mode: HIP-event ms per call (median of --steps), the library's stage table
per call (validate, layout, prune_small, prune_large / fast, repair, compact), the eight counts, the component size
histogram, the bit matrices' bytes, and `prune_step_us` = the prune_large stage over the largest component's vertex
count -- the stage runs every large component at once, one workgroup each, so this is the time per sequential step
of the largest one only where it dominates the stage (an upper bound otherwise).  Before timing the device's flags,
edges and counts are compared with the numpy restatement (tests/refs_model.py) bit for bit; `restatement_s` is that
restatement's time on the host.
--dump writes every network's largest components as edge lists; --stand-in times the REFERENCE's own loop, extracted
by tests/golden/make_golden_references.py, over its networkx stand-in for graph-tool (NOT graph-tool: networkx's
clique enumeration is another algorithm) on the largest dumped component it finishes within a minute.
No threshold is asserted here: the numbers are the record."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def networks(torch, engine, models, refine, synth):
    from tools.bench_assign import boundary_at_fraction
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n = 10_000
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    xs = (dist / dist.amax(dim=0)).contiguous()
    del dist
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0).astype(np.float64)
    m1 = np.quantile(sample, 0.30, axis=0).astype(np.float64)
    x, y, _ = refine.refineFit(refine.DeviceScorer(xs), [str(k) for k in range(n)], m0, m1, np.array([1.0, 1.0]), 0.0, 0.0)
    edges = engine.edge_threshold_dev(xs, 2, float(x), float(y))
    del xs
    yield "bench10k", edges.contiguous(), n, {"boundary_scaled": [float(x), float(y)]}

    allsk = synth.make_sketches_device(60_000, kmers, device="cuda:0", seed=synth.DEFAULT_SEED + 4)
    ref = engine.SketchDB(allsk[:n].contiguous(), 16, 14, device=0)
    qry = engine.SketchDB(allsk[n:].contiguous(), 16, 14, device=0)
    del allsk
    sample = engine.dist(ref, qry, kmers, tbl, q_begin=0, q_end=512)[0][::97].cpu().numpy()
    x_max, y_max = boundary_at_fraction(sample, 0.02)
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max)
    edges, _ = model.edges_from_sketches(ref, None, kmers, tbl)
    ref.close()
    qry.close()
    yield "config4", edges.contiguous(), n, {"boundary": [x_max, y_max]}


def event_ms(torch, fn, steps):
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4)}


def measure(a):
    import torch
    import refs_model as rm
    from poppunk_amd import _lib, engine, models, refine, synth
    from tools.bench_network import stage_table
    lib = _lib.lib()
    res = {"version": lib.ppk_version().decode(), "steps": a.steps, "device": torch.cuda.get_device_name(0),
           "options": {k: _lib.get_option(k) for k in ("refs_scratch_mb", "refs_lds_bits")}, "networks": {}}
    for name, edges, n, extra in networks(torch, engine, models, refine, synth):
        _, labels = engine.network_stats_dev(edges, n, labels=True)
        lab = labels.cpu().numpy()
        sizes = np.bincount(lab)
        big = np.sort(sizes)[::-1]
        words = int(sum(int(s) * ((int(s) + 63) // 64) for s in sizes if s >= 3))
        row = dict(extra, vertices=n, edges=int(edges.shape[0]), components=int(len(sizes)),
                   largest_components=big[:8].tolist(), components_3_to_64=int(((sizes >= 3) & (sizes <= 64)).sum()),
                   components_over_64=int((sizes > 64).sum()), bit_matrix_bytes=words * 8)
        e_host = edges.cpu().numpy()
        for mode, fast in (("clique", False), ("fast", True)):
            got = engine.pick_references_dev(edges, n, fast=fast)
            t0 = time.perf_counter()
            want = rm.pick_refs(e_host, n, fast=fast)
            restated = time.perf_counter() - t0
            same = (np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
                    and got[2] == want[2])
            for _ in range(3):
                engine.pick_references_dev(edges, n, fast=fast)
            r = event_ms(torch, lambda: engine.pick_references_dev(edges, n, fast=fast), a.steps)
            lib.ppk_prof_stages_enable(1)
            stage_table(lib)
            for _ in range(a.steps):
                engine.pick_references_dev(edges, n, fast=fast)
            torch.cuda.synchronize()
            lib.ppk_prof_stages_enable(0)
            r["stages_ms_per_call"] = {s: round(v["ms"] / a.steps, 4) for s, v in stage_table(lib).items()}
            r.update(counts=got[2], equals_restatement=bool(same), restatement_s=round(restated, 3))
            if not fast and big[0] > 64:
                r["prune_step_us"] = round(r["stages_ms_per_call"].get("prune_large", 0.0) * 1e3 / int(big[0]), 4)
            row[mode] = r
        res["networks"][name] = row
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            order = np.argsort(sizes)[::-1]
            keep = {}
            for rank, c in enumerate(order[:12].tolist()):
                verts = np.flatnonzero(lab == c)
                if len(verts) < 3:
                    continue
                local = np.full(n, -1, dtype=np.int64)
                local[verts] = np.arange(len(verts))
                inside = e_host[lab[e_host[:, 0]] == c]
                keep["edges_%d" % rank] = np.unique(np.sort(local[inside], axis=1), axis=0)
                keep["n_%d" % rank] = np.int64(len(verts))
            np.savez_compressed(os.path.join(a.dump, "components_%s.npz" % name), **keep)
    return res


def _stand_in_one(n, edges, queue):
    import contextlib
    import io
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_references as mgr
    ns = mgr.reference_namespace()
    sys.setrecursionlimit(20000)          # (cliquePrune sets 3 000 itself; the stand-in's frames sit on top of it)
    g = mgr._Graph()
    g.add_vertex(n)
    g.add_edge_list([tuple(e) for e in edges.tolist()])
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stderr(io.StringIO()):
        t0 = time.perf_counter()
        idx = ns["extractReferences"](g, ["s%d" % v for v in range(n)], tmp)[0]
        queue.put((time.perf_counter() - t0, len(idx)))


def stand_in(a):
    """the reference's loop over the networkx stand-in, component by component from the largest down, each in a child
    process that is ended after a minute: stops at the first one that finishes"""
    import multiprocessing as mp
    import refs_model as rm
    ctx = mp.get_context("fork")
    res = {"what": "PopPUNK/network.py extractReferences over a networkx stand-in for graph-tool, one component, host CPU",
           "limit_s": 60}
    for fname in sorted(os.listdir(a.stand_in)):
        if not (fname.startswith("components_") and fname.endswith(".npz")):
            continue
        with np.load(os.path.join(a.stand_in, fname)) as f:
            comps = sorted(((int(f[k]), f["edges_" + k[2:]]) for k in f.files if k.startswith("n_")), key=lambda t: -t[0])
        rows, seen = [], set()
        for n, edges in comps:
            if n in seen:
                continue
            seen.add(n)
            queue = ctx.Queue()
            child = ctx.Process(target=_stand_in_one, args=(n, edges, queue))
            child.start()
            child.join(60.0)
            finished = not child.is_alive()
            if not finished:
                child.terminate()
                child.join()
            t0 = time.perf_counter()
            ours = rm.pick_refs(edges, n)[2]["references"]
            row = {"vertices": n, "edges": int(len(edges)), "finished": finished,
                   "restatement_s": round(time.perf_counter() - t0, 4), "rule_references": ours}
            if finished and not queue.empty():
                took, picked = queue.get()
                row.update(stand_in_s=round(took, 3), stand_in_references=picked)
            rows.append(row)
            if finished:
                break
        res[fname[len("components_"):-4]] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--stand-in", default=None)
    a = ap.parse_args()
    res = stand_in(a) if a.stand_in else measure(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
