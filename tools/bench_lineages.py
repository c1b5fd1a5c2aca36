"""Lineages within every strain on the MI355X (ppk_strain_knn_dev, ppk_strain_ranks_dev).

    timeout -k 10 900 python tools/bench_lineages.py [--out profiles/lineages/bench_lineages.json]

bench.py's 10 000-genome matrix; the strains are the clusters of the refine-style sweep tools/bench_clusters.py uses
(40 boundaries of slope 2 from the 1 % to the 30 % quantile point), at the level whose cluster count is closest to the
200 strains the sketches were made from; --min-count 10, ranks 1,2,3, search depth 10 000 (the script's defaults).
Records, in one run on one build:
  one_pass    the two new calls and the cluster sweep over their stream: HIP-event ms per call (median of --steps after
              two warm-ups) and the library's stage split
  loop        the same result strain by strain through the calls that existed before: prune_long_dev ->
              long_to_square_dev -> ppk_knn_dev -> lowerRank per rank (host arrays) -> cluster numbers per rank; wall
              ms, one pass after a warm-up pass (it takes seconds)
  pure_read   torch.sum of the matrix
and whether the loop and the one pass give the same arrays.  No threshold is asserted: the numbers are the record."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10_000)
    ap.add_argument("--min-count", type=int, default=10)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, network, poppunk_refine, synth
    lib = _lib.lib()
    n = a.samples
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    xs = (dist / dist.amax(dim=0)).contiguous()
    sample = xs[::20].cpu().numpy()
    m0, m1 = np.quantile(sample, 0.01, axis=0), np.quantile(sample, 0.30, axis=0)
    offs = np.ascontiguousarray(np.linspace(0.0, float(np.linalg.norm(m1 - m0)), 40), dtype=np.float64)
    i, j, o = engine.threshold_iterate_1d_dev(xs, offs, 2, m0[0], m0[1], m1[0], m1[1])
    del xs
    levels_t, counts = engine.cluster_sweep_dev(i, j, o, n, 40)
    counts = counts.cpu().numpy()
    level = int(np.argmin(np.abs(counts - n // 50)))
    labels = levels_t[level].cpu().numpy()
    # strains in number order, members in a shuffled (CSV-like) order; those below min_count are left out
    rng = np.random.default_rng(1)
    order = rng.permutation(n)
    groups = {}
    for g in order:
        groups.setdefault(int(labels[g]), []).append(int(g))
    kept = [np.asarray(groups[c], dtype=np.int64) for c in sorted(groups) if len(groups[c]) >= a.min_count]
    members = np.concatenate(kept)
    seg_off = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    sizes = np.diff(seg_off)
    ranks, depth = [1, 2, 3], 10_000
    members_t = torch.as_tensor(members, device=dist.device)
    m = int(seg_off[-1])
    res = {"version": lib.ppk_version().decode(), "samples": n, "level": level, "clusters_at_level": int(counts[level]),
           "strains_kept": len(kept), "members": m, "largest_strain": int(sizes.max()),
           "strains_by_route": {"wave": int((sizes <= 65).sum()), "lds": int(((sizes > 65) & (sizes <= 4097)).sum()),
                                "long": int((sizes > 4097).sum())},
           "list_entries": engine.strain_nnz(seg_off, depth), "ranks": ranks, "steps": a.steps,
           "options": {k: _lib.get_option(k) for k in ("lineage_scratch_mb", "lineage_lds_keys")}}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return {"median_ms": round(t[len(t) // 2], 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5)}

    def stages(fn):
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        return {k: round(v["ms"] / a.steps, 4) for k, v in stage_table(lib).items()}

    knn = lambda: engine.strain_knn_dev(dist, members_t, seg_off, depth, 0)
    oi, oj, od = knn()
    rank_call = lambda: engine.strain_ranks_dev(oj, od, seg_off, depth, ranks)
    prefix, pi, pj, lv, sd = rank_call()
    sweep = lambda: engine.cluster_sweep_dev(pi, pj, lv, m, len(ranks))

    def one_pass():
        a_, b_, c_ = knn()
        p_ = engine.strain_ranks_dev(b_, c_, seg_off, depth, ranks)
        return engine.cluster_sweep_dev(p_[1], p_[2], p_[3], m, len(ranks))
    res["one_pass"] = {"strain_knn_dev": timed(knn), "strain_knn_dev_stages_ms": stages(knn),
                       "strain_ranks_dev": timed(rank_call), "strain_ranks_dev_stages_ms": stages(rank_call),
                       "cluster_sweep_dev": timed(sweep), "all_three": timed(one_pass), "stream_entries": int(pi.shape[0])}
    res["pure_read"] = timed(lambda: torch.sum(dist))
    print("one_pass", json.dumps(res["one_pass"]), flush=True)

    numbers = engine.strain_cluster_numbers(sweep()[0], seg_off).cpu().numpy()
    h_oj, h_od, h_prefix = oj.cpu().numpy(), od.cpu().numpy(), prefix.cpu().numpy()
    out_off = np.concatenate([[0], np.cumsum(sizes * np.minimum(depth, sizes - 1))])
    vp = C.c_void_p

    def loop(check):
        same = True
        for s, mem in enumerate(kept):
            n_s = len(mem)
            keep = np.sort(mem)
            sq = engine.long_to_square_dev(engine.prune_long_dev(dist, n, keep), 0, n_s)
            at = torch.as_tensor(np.searchsorted(keep, mem), device=dist.device)
            sq = sq[at][:, at].contiguous()                      # the strain's local order
            d_s = n_s - 1
            ti = torch.empty(n_s * d_s, dtype=torch.int64, device=dist.device)
            tj, td = torch.empty_like(ti), torch.empty(n_s * d_s, dtype=torch.float32, device=dist.device)
            _lib.check(lib.ppk_knn_dev(vp(sq.data_ptr()), n_s, d_s, vp(ti.data_ptr()), vp(tj.data_ptr()),
                                       vp(td.data_ptr()), None), "ppk_knn_dev")
            hi, hj, hd = ti.cpu().numpy(), tj.cpu().numpy(), td.cpu().numpy()
            if check:
                same = same and np.array_equal(hj, h_oj[out_off[s]:out_off[s + 1]]) and np.array_equal(
                    hd.view(np.uint32), h_od[out_off[s]:out_off[s + 1]].view(np.uint32))
            for q, rank in enumerate(ranks):
                li, lj, _ = poppunk_refine.lowerRank_arrays((hi, hj, hd), n_s, rank, False, False, 1e-10, 1)
                nums = network.cluster_numbers((np.stack([li, lj], axis=1), n_s))
                if check:
                    same = same and np.array_equal(np.bincount(li, minlength=n_s), h_prefix[q, seg_off[s]:seg_off[s + 1]])
                    same = same and np.array_equal(nums, numbers[q, seg_off[s]:seg_off[s + 1]])
        torch.cuda.synchronize()
        return bool(same)

    loop(False)
    t0 = time.perf_counter()
    loop(False)
    wall = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    one_pass()
    torch.cuda.synchronize()
    res["one_pass"]["all_three_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["loop"] = {"wall_ms": round(wall, 1), "same_arrays_as_one_pass": loop(True)}
    res["loop_over_one_pass"] = round(wall / res["one_pass"]["all_three_wall_ms"], 1)
    res["one_pass_over_pure_read"] = round(res["one_pass"]["all_three"]["median_ms"] / res["pure_read"]["median_ms"], 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
