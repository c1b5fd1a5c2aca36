"""A query batch added to the lineages of every strain on the MI355X (ppk_strain_extend_dev, ppk_strain_ranks_dev on
its lists).

    timeout -k 10 900 python tools/bench_lineage_query.py [--out profiles/lineage_query/bench_lineage_query.json]

The references are tools/bench_lineages.py's: bench.py's 10 000-genome matrix, its strains of at least 10 members, the
stored neighbour lists at search depth 10 000 (ppk_strain_knn_dev's, floored at 1e-10 as a saved model holds them),
ranks 1,2,3.  The batch is --queries (1 000) queries, each placed on a template member drawn uniformly from the members
of those strains, so every strain's share follows its size: a query's distances are its template's, stretched by a
factor in [1, 1.05) of its own per pair (to the template itself: half the template's distance to the next sample);
every tenth query is an exact copy of its template (distance 0 to it: the floor, and runs of equal distances across the
two sides).  Both matrices are built on the device from the resident reference matrix; sketching the queries is not
what is measured.
Records, in one run on one build:
  one_pass    strain_extend_dev, strain_ranks_dev on its lists, cluster_sweep_dev + strain_cluster_numbers: HIP-event ms
              per call (median of --steps after two warm-ups), the library's stage split, and all three together
  loop        the same result strain by strain through the calls that existed before (ppk_extend, ppk_lower_rank per
              rank, cluster numbers per rank: LineageRanks.extend's steps and printClusters' numbers), the strain's
              square and rectangle cut out of host copies of the two matrices; wall ms, one pass after a warm-up pass
  pure_read   torch.sum of the two matrices
and whether the loop and the one pass give the same arrays.  No threshold is asserted: the numbers are the record."""
import argparse
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
    ap.add_argument("--queries", type=int, default=1_000)
    ap.add_argument("--min-count", type=int, default=10)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, lineages, models, synth
    lib = _lib.lib()
    n, nq = a.samples, a.queries
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sk, _ = synth.make_sketches(n, kmers, cluster_size=50)
    db = engine.SketchDB(sk, 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    dev = dist.device
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
    members_t = torch.as_tensor(members, device=dev)
    _, nn_j, nn_d = engine.strain_knn_dev(dist, members_t, seg_off, depth, 0)
    nn_d = nn_d.clamp_min(float(np.float32(models.EPSILON)))

    # the batch: templates, the strain of each, and the two matrices from the reference matrix, on the device
    place = np.sort(rng.integers(0, len(members), nq))           # positions in the member array
    strain_of = np.searchsorted(seg_off, place, side="right") - 1
    shuffle = rng.permutation(nq)                                # query ids interleave across strains
    template = np.empty(nq, dtype=np.int64)
    template[shuffle] = members[place]
    queries = shuffle.astype(np.int64)                           # strain by strain, ids not ascending
    qry_off = np.concatenate([[0], np.cumsum(np.bincount(strain_of, minlength=len(kept)))]).astype(np.int64)
    t_t = torch.as_tensor(template, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    def long_rows(a_t, b_t):
        lo, hi = torch.minimum(a_t, b_t), torch.maximum(a_t, b_t)
        same = lo == hi
        hi = torch.where(same, (lo + 1) % n, hi)
        lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
        rows = dist[lo * (2 * n - lo - 1) // 2 + (hi - lo - 1)]
        return rows, same                 # (a sample against itself: its distance to the next sample stands in)
    refs = torch.arange(n, device=dev)
    qr, same = long_rows(t_t[:, None].expand(nq, n).reshape(-1), refs[None, :].expand(nq, n).reshape(-1))
    stretch = 1 + 0.05 * torch.rand(qr.shape, generator=gen, device=dev)
    exact = (torch.arange(nq, device=dev) % 10 == 0)[:, None].expand(nq, n).reshape(-1)
    qr = torch.where(exact[:, None], torch.where(same[:, None], torch.zeros_like(qr), qr),
                     qr * stretch * torch.where(same, 0.5, 1.0)[:, None]).contiguous()
    qa, qb = torch.triu_indices(nq, nq, 1, device=dev)
    qq, same = long_rows(t_t[qa], t_t[qb])
    qq = (qq * (1 + 0.05 * torch.rand(qq.shape, generator=gen, device=dev)) * torch.where(same, 0.5, 1.0)[:, None])
    qq = qq.to(torch.float32).contiguous()
    qr = qr.to(torch.float32)
    del stretch, exact, qa, qb, same
    queries_t = torch.as_tensor(queries, device=dev)
    ext_off = seg_off + qry_off
    ext_sizes = np.diff(ext_off)
    m_x = int(ext_off[-1])
    res = {"version": lib.ppk_version().decode(), "samples": n, "queries": nq, "strains": len(kept),
           "strains_with_queries": int((np.diff(qry_off) > 0).sum()), "members": int(seg_off[-1]),
           "largest_extended_strain": int(ext_sizes.max()), "most_queries_in_a_strain": int(np.diff(qry_off).max()),
           "strains_by_route": {"wave": int((ext_sizes <= 65).sum()),
                                "lds": int(((ext_sizes > 65) & (ext_sizes <= 4097)).sum()),
                                "long": int((ext_sizes > 4097).sum())},
           "stored_entries": int(nn_j.shape[0]), "list_entries": engine.strain_nnz(ext_off, depth), "ranks": ranks,
           "steps": a.steps, "options": {k: _lib.get_option(k) for k in ("lineage_scratch_mb", "lineage_lds_keys")}}

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

    extend = lambda: engine.strain_extend_dev(members_t, seg_off, queries_t, qry_off, nn_j, nn_d, qr, qq, n, nq, depth,
                                              0, models.EPSILON)
    oi, oj, od = extend()
    rank_call = lambda: engine.strain_ranks_dev(oj, od, ext_off, depth, ranks)
    prefix, pi, pj, lv, sd = rank_call()
    sweep = lambda: engine.strain_cluster_numbers(engine.cluster_sweep_dev(pi, pj, lv, m_x, len(ranks))[0], ext_off)

    def one_pass():
        a_, b_, c_ = extend()
        p_ = engine.strain_ranks_dev(b_, c_, ext_off, depth, ranks)
        return engine.strain_cluster_numbers(engine.cluster_sweep_dev(p_[1], p_[2], p_[3], m_x, len(ranks))[0], ext_off)
    res["one_pass"] = {"strain_extend_dev": timed(extend), "strain_extend_dev_stages_ms": stages(extend),
                       "strain_ranks_dev": timed(rank_call), "strain_ranks_dev_stages_ms": stages(rank_call),
                       "cluster_sweep_and_numbers": timed(sweep), "all_three": timed(one_pass),
                       "stream_entries": int(pi.shape[0])}
    res["pure_read"] = timed(lambda: (torch.sum(qr), torch.sum(qq)))
    print("one_pass", json.dumps(res["one_pass"]), flush=True)

    numbers = sweep().cpu().numpy()
    h_oj, h_od, h_prefix = oj.cpu().numpy(), od.cpu().numpy(), prefix.cpu().numpy()
    out_off = np.concatenate([[0], np.cumsum(ext_sizes * np.minimum(depth, ext_sizes - 1))])
    nn_off = np.concatenate([[0], np.cumsum(sizes * np.minimum(depth, sizes - 1))])
    h_nn_j, h_nn_d = nn_j.cpu().numpy(), nn_d.cpu().numpy()
    h_qr, h_qq = qr.cpu().numpy(), qq.cpu().numpy()
    stored = []
    for s, mem in enumerate(kept):
        n_s = len(mem)
        old = models.LineageRanks(ranks, depth)
        rows = np.repeat(np.arange(n_s), min(depth, n_s - 1))
        old.nn_dists = old._coo(h_nn_d[nn_off[s]:nn_off[s + 1]], rows, h_nn_j[nn_off[s]:nn_off[s + 1]], n_s)
        old.fitted = True
        stored.append(old)

    def loop(check):
        same = True
        for s, mem in enumerate(kept):
            qry = queries[qry_off[s]:qry_off[s + 1]]
            if not len(qry):
                continue
            model, nums = lineages._extend_alone(stored[s], models.LineageRanks(ranks, depth), mem, qry, h_qr, h_qq, n, nq)
            if check:
                n_x = len(mem) + len(qry)
                same = same and np.array_equal(model.nn_dists.col, h_oj[out_off[s]:out_off[s + 1]]) and np.array_equal(
                    model.nn_dists.data.view(np.uint32), h_od[out_off[s]:out_off[s + 1]].view(np.uint32))
                for q, rank in enumerate(ranks):
                    same = same and np.array_equal(np.bincount(model.lower_rank_dists[rank].row, minlength=n_x),
                                                   h_prefix[q, ext_off[s]:ext_off[s + 1]])
                    same = same and np.array_equal(nums[q], numbers[q, ext_off[s]:ext_off[s + 1]])
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
    assert res["loop"]["same_arrays_as_one_pass"], "the loop and the one pass differ"
    res["loop_over_one_pass"] = round(wall / res["one_pass"]["all_three_wall_ms"], 1)
    res["one_pass_over_pure_read"] = round(res["one_pass"]["all_three"]["median_ms"] / res["pure_read"]["median_ms"], 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
