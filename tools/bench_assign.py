"""Query assignment on the MI355X (ppk_cluster_extend_dev, ppk_query_links_dev) on BASELINE config
4's shape with bench.py's generator: ONE population of 60 000 synthetic genomes, the first 10 000 the reference
database, the other 50 000 the queries; a slope-2 boundary with 2 % of the query-reference pairs inside; the reference
network is the model's own self edges of the 10 000.

    timeout -k 10 600 python tools/bench_assign.py [--out profiles/assign/bench_assign.json]

Records, HIP-event ms per call, median of --steps, all in one run, the routes taken in turn within every step:
  extend        cluster_extend_dev over the new edges and the reference components' labels
  full_graph    the route without it: torch.cat of the reference edges and the new edges, then cluster_numbers_dev
  links_ordered / links_shuffled   query_links_dev (max_links 8) on the stream as the fused path emits it, and on a
                random permutation of it (the sort route)
  serial_sample the reference's `serial` way for a sample of 64 queries: per query, the reference edges + its own
                edges, one cluster_numbers_dev; `per_query_ms` is measured, `all_queries_s` is that times 50 000 --
                an EXTRAPOLATION, not a measurement
with the library's stage split for the calls, and `outside_stages_ms` = the median minus the stages: the read-backs a
call waits for (the ordered links route has two, the second for the overflow list's length) and launch gaps.  The
two routes' numbers are compared bit for bit before timing.
No threshold is asserted here: the numbers are the record."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table      # noqa: E402


def boundary_at_fraction(sample, frac):
    """bench.py's _boundary_at_fraction: the triangle through the medians of the two columns, scaled to the `frac`
    quantile of x / x_med + y / y_med"""
    d = np.asarray(sample, dtype=np.float64)
    xm, ym = max(float(np.median(d[:, 0])), 1e-6), max(float(np.median(d[:, 1])), 1e-6)
    t = float(np.quantile(d[:, 0] / xm + d[:, 1] / ym, frac))
    return t * xm, t * ym


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--refs", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=50000)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, models, synth
    lib = _lib.lib()
    dev = "cuda:0"
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n_ref, n_qry = a.refs, a.queries
    allsk = synth.make_sketches_device(n_ref + n_qry, kmers, device=dev, seed=synth.DEFAULT_SEED + 4)
    ref = engine.SketchDB(allsk[:n_ref].contiguous(), 16, 14, device=0)
    qry = engine.SketchDB(allsk[n_ref:].contiguous(), 16, 14, device=0)
    del allsk
    sample = engine.dist(ref, qry, kmers, tbl, q_begin=0, q_end=min(n_qry, 512))[0][::97].cpu().numpy()
    x_max, y_max = boundary_at_fraction(sample, 0.02)
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max)
    ref_edges, _ = model.edges_from_sketches(ref, None, kmers, tbl)
    new, _ = model.edges_from_sketches(ref, qry, kmers, tbl)
    ref.close()
    qry.close()
    stats, labels = engine.network_stats_dev(ref_edges, n_ref, labels=True)
    n = n_ref + n_qry
    res = {"version": lib.ppk_version().decode(), "refs": n_ref, "queries": n_qry, "steps": a.steps,
           "boundary": [x_max, y_max], "reference_edges": int(ref_edges.shape[0]),
           "reference_components": int(stats[1].item()), "new_edges": int(new.shape[0])}
    shuffled = new[torch.randperm(new.shape[0], device=dev)].contiguous()

    routes = {
        "extend": lambda: engine.cluster_extend_dev(new, labels, n_qry),
        "full_graph": lambda: engine.cluster_numbers_dev(torch.cat([ref_edges, new]), n),
        "links_ordered": lambda: engine.query_links_dev(new, labels, n_qry, 8),
        "links_shuffled": lambda: engine.query_links_dev(shuffled, labels, n_qry, 8),
    }
    a_num, a_cnt = routes["extend"]()
    b_num, b_cnt = routes["full_graph"]()
    res["extend_equals_full_graph"] = bool(torch.equal(a_num, b_num)) and a_cnt == b_cnt
    res["clusters"] = a_cnt
    lo, ls = routes["links_ordered"](), routes["links_shuffled"]()
    res["links_shuffled_equals_ordered"] = all(bool(torch.equal(x, y)) for x, y in zip(lo, ls))
    res["unlinked_queries"] = int((lo[0] == 0).sum().item())
    res["queries_linked_to_more_than_one_component"] = int((lo[1] > 1).sum().item())
    res["max_components_per_query"] = int(lo[1].max().item())

    for _ in range(3):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(a.steps):
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    for k, t in times.items():
        t = sorted(t)
        res[k] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}
    for k in ("extend", "full_graph", "links_ordered", "links_shuffled"):
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        for _ in range(a.steps):
            routes[k]()
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        res[k]["stages_ms_per_call"] = {s: round(v["ms"] / a.steps, 4) for s, v in stage_table(lib).items()}
        # what the call spends outside its stages: the read-backs it waits for (links_ordered: two, the second for the
        # overflow list's length) and launch gaps
        res[k]["outside_stages_ms"] = round(res[k]["median_ms"] - sum(res[k]["stages_ms_per_call"].values()), 4)
    res["full_graph_over_extend"] = round(res["full_graph"]["median_ms"] / res["extend"]["median_ms"], 2)

    # the reference's serial way for 64 queries: the whole reference network + one query's edges, components, per query
    qs = torch.linspace(0, n_qry - 1, 64, device=dev).long()
    per_query = []
    for q in qs.tolist():
        mine = new[new[:, 1] == n_ref + q].clone()
        mine[:, 1] = n_ref
        per_query.append(mine)
    torch.cuda.synchronize()

    def serial():
        for mine in per_query:
            engine.cluster_numbers_dev(torch.cat([mine, ref_edges]), n_ref + 1)
    serial()
    t = []
    for _ in range(max(3, a.steps // 2)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        serial()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    t = sorted(t)
    per = t[len(t) // 2] / 64
    res["serial_sample"] = {"queries": 64, "per_query_ms": round(per, 4),
                            "all_queries_s": round(per * n_qry / 1e3, 2),
                            "what": "all_queries_s = per_query_ms x the query count: an extrapolation, not a measurement"}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
