"""Network betweenness on the MI355X (ppk_network_summary_dev): bench.py's 10 000-genome matrix and
its 40-offset thresholdIterate1D sweep (built as tools/bench_network.py builds it), scored with exact betweenness.

    timeout -k 10 900 python tools/bench_betweenness.py [--out profiles/betweenness/bench_betweenness.json]
                                                        [--final-only] [--steps K] [--no-cpu]
                                                        [--sampled K] [--seed S]

Records: HIP-event ms and wall ms per call (median of --steps after one warm-up) for the final graph alone (every
edge at one offset: what each fit's networkSummary pays) and, unless --final-only, for the whole sweep; the library's
stage split of each; the work model W = sum over components c of more than 3 vertices of n_c * (adjacency entries of
c) per graph, and the probe rate 2 W / time it implies (each source reads every row of its component twice: discover
with sigma, then delta); the final graph's component sizes and betweenness means.  CPU: networkx cannot finish the
final graph in reasonable time, so a networkx Brandes of one subgraph is timed and EXTRAPOLATED by the work model.
--sampled K (default 100; 0 leaves the leg out): the sampled call (ppk_network_summary_sampled_dev, at most K sources
per component) timed next to the exact call in the same run, with its stage split, |sampled - exact| of the two
betweenness means per level, and whether grow_scores(score_idx = 1 and 2) puts its optimum at the same level.
--pmc-only: only final-graph calls (five), the program a counter pass (rocprofv3 --pmc) runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table  # noqa: E402


def sweep_edges():
    """bench.py's scaled 10 000-genome matrix and its 40-offset sweep (tools/bench_network.py)"""
    import torch  # noqa: F401
    from poppunk_amd import engine, synth
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(10_000, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    db.close()
    scale = dist.amax(dim=0)
    xs = (dist / scale).contiguous()
    del dist
    sample = xs[::20].cpu().numpy()
    m0 = np.quantile(sample, 0.01, axis=0)
    m1 = np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    return engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])


def work_model(ih, jh, n):
    """(sum over components of > 3 vertices of n_c * adjacency entries, their sizes) of one graph"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    A = coo_matrix((np.ones(ih.size, dtype=np.int8), (ih, jh)), shape=(n, n))
    _, lab = connected_components(A, directed=False)
    sizes = np.bincount(lab)
    adj = np.bincount(lab[ih], minlength=sizes.size) * 2
    big = sizes > 3
    return int((sizes[big].astype(np.int64) * adj[big]).sum()), sorted(sizes[big].tolist(), reverse=True)


def timed(call, steps):
    import torch
    call()
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
    return round(float(np.median(evs)), 3), round(float(np.median(wall)), 3)


def staged(lib, call, steps):
    import torch
    lib.ppk_prof_stages_enable(1)
    stage_table(lib)
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    lib.ppk_prof_stages_enable(0)
    st = stage_table(lib)
    return {k: round(v["ms"] / steps, 4) for k, v in st.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--final-only", action="store_true")
    ap.add_argument("--pmc-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--sampled", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine
    lib = _lib.lib()
    i, j, o = sweep_edges()
    n, m = 10_000, int(i.shape[0])

    def final():
        return engine.network_summary_dev(i, j, None, n, 1)

    def sweep():
        return engine.network_summary_dev(i, j, o, n, 40)

    if a.pmc_only:
        for _ in range(5):
            final()
        torch.cuda.synchronize()
        print("pmc-only: 5 final-graph calls, %d edges" % m)
        return
    res = {"version": lib.ppk_version().decode(), "samples": n, "offsets": 40, "edges": m, "steps": a.steps}
    ih, jh, oh = i.cpu().numpy(), j.cpu().numpy(), o.cpu().numpy()
    w_final, sizes = work_model(ih, jh, n)
    ev, wall = timed(final, a.steps)
    stats, bt, scored, _ = final()
    res["final"] = {"event_ms": ev, "wall_ms": wall, "stages_ms_per_call": staged(lib, final, a.steps),
                    "work_model": w_final, "probes_per_s": round(2 * w_final / (ev * 1e-3), -6),
                    "components_scored": int(scored[0]), "scored_sizes": sizes,
                    "counts": [int(x) for x in stats[0].tolist()], "bt": [float(x) for x in bt[0].tolist()]}
    print(json.dumps(res["final"]), flush=True)
    if not a.final_only:
        w_sweep = []
        for t in range(40):
            sel = oh <= t
            w_sweep.append(work_model(ih[sel], jh[sel], n)[0] if sel.any() else 0)
        ev, wall = timed(sweep, a.steps)
        _, bt_s, _, _ = sweep()
        assert torch.equal(bt_s[-1], bt[0]), "the sweep's last graph differs from the final graph"
        res["sweep"] = {"event_ms": ev, "wall_ms": wall, "stages_ms_per_call": staged(lib, sweep, a.steps),
                        "work_model_per_graph": w_sweep, "work_model": int(sum(w_sweep)),
                        "probes_per_s": round(2 * sum(w_sweep) / (ev * 1e-3), -6)}
        print(json.dumps({k: v for k, v in res["sweep"].items() if k != "work_model_per_graph"}), flush=True)
    if a.sampled > 0:
        from poppunk_amd import refine

        def final_s():
            return engine.network_summary_sampled_dev(i, j, None, n, 1, sources=a.sampled, seed=a.seed)

        def sweep_s():
            return engine.network_summary_sampled_dev(i, j, o, n, 40, sources=a.sampled, seed=a.seed)

        ev, wall = timed(final_s, a.steps)
        stats_s, bt_f, _, _ = final_s()
        assert torch.equal(stats_s, stats), "the sampled call's counts differ"
        leg = {"sources": a.sampled, "seed": a.seed,
               "final": {"event_ms": ev, "wall_ms": wall, "stages_ms_per_call": staged(lib, final_s, a.steps),
                         "exact_event_ms": res["final"]["event_ms"],
                         "speedup": round(res["final"]["event_ms"] / ev, 2), "bt": [float(x) for x in bt_f[0].tolist()],
                         "abs_diff_bt": [abs(float(x) - float(y)) for x, y in zip(bt_f[0].tolist(), bt[0].tolist())]}}
        if not a.final_only:
            ev, wall = timed(sweep_s, a.steps)
            st_s, bt_ss, _, _ = sweep_s()
            diff = (bt_ss - bt_s).abs().cpu().numpy()
            st_h = st_s.cpu().numpy()
            optimum = {}
            for idx in (1, 2):
                ex = refine.grow_scores(st_h, n, idx, bt=bt_s.cpu().numpy())
                sa = refine.grow_scores(st_h, n, idx, bt=bt_ss.cpu().numpy())
                optimum["score_idx_%d" % idx] = {"exact_level": int(np.argmin(ex)), "sampled_level": int(np.argmin(sa)),
                                                 "same": bool(np.argmin(ex) == np.argmin(sa)),
                                                 "max_abs_score_diff": float(np.abs(np.array(ex) - np.array(sa)).max())}
            leg["sweep"] = {"event_ms": ev, "wall_ms": wall, "stages_ms_per_call": staged(lib, sweep_s, a.steps),
                            "exact_event_ms": res["sweep"]["event_ms"],
                            "speedup": round(res["sweep"]["event_ms"] / ev, 2),
                            "abs_diff_mean_per_level": [float(x) for x in diff[:, 0]],
                            "abs_diff_weighted_mean_per_level": [float(x) for x in diff[:, 1]],
                            "max_abs_diff": [float(diff[:, 0].max()), float(diff[:, 1].max())], "optimum": optimum}
        res["sampled"] = leg
        print(json.dumps(leg), flush=True)
    if not a.no_cpu:
        # networkx Brandes of the subgraph on the first k vertices of the largest component, extrapolated by W
        import networkx as nx
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, lab = connected_components(coo_matrix((np.ones(m, dtype=np.int8), (ih, jh)), shape=(n, n)), directed=False)
        big = np.flatnonzero(lab == np.bincount(lab).argmax())[:160]
        keep = np.isin(ih, big) & np.isin(jh, big)
        g = nx.Graph()
        g.add_edges_from(zip(ih[keep].tolist(), jh[keep].tolist()))
        g = g.subgraph(max(nx.connected_components(g), key=len)).copy()
        w_sub = g.number_of_nodes() * 2 * g.number_of_edges()
        t0 = time.perf_counter()
        nx.betweenness_centrality(g, normalized=True)
        cpu_s = time.perf_counter() - t0
        res["cpu_extrapolation"] = {
            "what": "networkx betweenness_centrality (one thread) of a %d-vertex, %d-edge subgraph of the final "
                    "graph's largest component, EXTRAPOLATED to the final graph by the work model (not run on it)"
                    % (g.number_of_nodes(), g.number_of_edges()),
            "seconds_subgraph": round(cpu_s, 3), "work_model_subgraph": w_sub,
            "seconds_final_graph_extrapolated": round(cpu_s * w_final / w_sub, 1)}
        if "sweep" in res:
            res["cpu_extrapolation"]["seconds_sweep_extrapolated"] = round(cpu_s * res["sweep"]["work_model"] / w_sub, 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
