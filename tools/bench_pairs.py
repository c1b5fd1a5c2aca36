"""Pair-list distances on the MI355X (ppk_dist_pairs_dev) at 100 000 genomes, s = 1 024, sketches
drawn on the device (synth.make_sketches_device), against the full ppk_dist_dev pass measured in the same run.

    timeout -k 10 900 python tools/bench_pairs.py [--out profiles/pairs/bench_pairs.json]

Records, per list, the stage times of one warm call summed from ppk_prof_stages_read (pairs_check, pairs_image,
pairs_counts, pairs_fit), the HIP-event time of the whole call, pairs per second and the ratio to the full pass:
  sampled       100 000 pairs from models.sample_rows(seed 42): the rows a fit trains on.  The only other route to those
                rows is the pass into a 40 GB matrix plus a gather; the rows of both are compared bit for bit here.
                Also the device memory the call took beyond the database (free memory before and after, outputs
                included; the scratch is grow-only, so what the call took is still held afterwards).
  edges         row-ordered fused edge lists (engine.dist_edges, a core-distance threshold at the quantile that gives
                about 1e5, 1e6, 1e7 and 1e8 edges).
No threshold is asserted here: the numbers are the record."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table      # noqa: E402

STAGES = ("pairs_check", "pairs_image", "pairs_counts", "pairs_fit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--edges", default="1e5,1e6,1e7,1e8")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, models, synth
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    n = a.samples
    n_rows = n * (n - 1) // 2
    t = synth.make_sketches_device(n, kmers, device="cuda:0")
    db = engine.SketchDB(t, 16, 14)
    del t
    torch.cuda.empty_cache()
    res = {"version": lib.ppk_version().decode(), "samples": n, "rows": n_rows,
           "pairs_scratch_mb": _lib.get_option("pairs_scratch_mb"), "lists": {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def list_call(pairs_t):
        engine.dist_pairs(db, None, kmers, tbl, pairs_t)          # warm: scratch and tables are there
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        (out, _), ms = event_ms(lambda: engine.dist_pairs(db, None, kmers, tbl, pairs_t))
        st = stage_table(lib)
        lib.ppk_prof_stages_enable(0)
        stages = {k: st.get(k, {"ms": 0.0})["ms"] for k in STAGES}
        total = sum(stages.values())
        m = int(pairs_t.shape[0])
        return out, {"pairs": m, "stages_ms": stages, "stages_sum_ms": round(total, 4), "call_ms": round(ms, 4),
                     "pairs_per_s": round(m / (total * 1e-3)), "share_of_all_pairs": m / n_rows}

    # (a) the sampled list, before the matrix exists
    rows = models.sample_rows(n_rows, 100_000, 42)
    pairs_t = torch.as_tensor(engine.rows_to_pairs(rows, n), device=dev)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    got, rec = list_call(pairs_t)
    free1, _ = torch.cuda.mem_get_info(0)
    rec["device_bytes_taken"] = int(free0 - free1)
    res["lists"]["sampled"] = rec

    # the full pass, twice (the second is the figure), and the same rows gathered from it
    dense, _ = engine.dist(db, None, kmers, tbl)
    (dense, _), pass_ms = event_ms(lambda: engine.dist(db, None, kmers, tbl, out=dense))
    res["full_pass_ms"] = round(pass_ms, 3)
    idx_t = torch.as_tensor(rows, device=dev)
    want, gather_ms = event_ms(lambda: dense[idx_t])
    res["gather_ms"] = round(gather_ms, 4)
    res["sampled_rows_equal_dense"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    rec["full_pass_over_list"] = round((pass_ms + gather_ms) / rec["stages_sum_ms"], 2)

    # boundaries of (b): core-distance quantiles from a sample of the matrix
    probe = dense[torch.randint(0, n_rows, (4_000_000,), device=dev, generator=torch.Generator(dev).manual_seed(1))][:, 0]
    probe = probe.sort().values
    del dense, want
    torch.cuda.empty_cache()
    for want_edges in [float(x) for x in a.edges.split(",")]:
        q = want_edges / n_rows
        x_max = float(probe[min(int(q * probe.numel()), probe.numel() - 1)].item())
        edges, _ = engine.dist_edges(db, None, kmers, tbl, slope=0, x_max=x_max, y_max=0.0, cap=int(want_edges * 2) + 1024)
        if edges.shape[0] == 0:
            continue
        _, rec = list_call(edges)
        rec["x_max"] = x_max
        rec["full_pass_over_list"] = round(pass_ms / rec["stages_sum_ms"], 3)
        res["lists"]["edges_%g" % want_edges] = rec
        del edges
        torch.cuda.empty_cache()

    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
