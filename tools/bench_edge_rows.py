"""Fused edge lists that carry their distances on the MI355X (ppk_dist_edges_rows_dev), against
today's calls measured in the same run, s = 1 024, sketches drawn on the device (synth.make_sketches_device).

    timeout -k 10 1100 python tools/bench_edge_rows.py [--out profiles/edge_rows/bench_edge_rows.json] [--shapes 10k,100k,config4]

Per shape, four legs, each the median HIP-event time of --reps warm calls in ONE process:
  (a) ppk_dist_edges_dev alone                          today's fused edge list
  (b) ppk_dist_edges_rows_dev                           the new call (ppk_last_kernel_name recorded: fused or two-step)
  (c) (a) followed by ppk_dist_pairs_dev on its edges   today's way to the rows
  (d) ppk_dist_dev into the matrix                      (skipped where the matrix does not fit: 100k needs 40 GB)
and the same (b) with option edge_rows_fused 0 (the two-step inside the entry point).  Reported: (b) - (a), the price of
the rows, and (c) / (b), what they save; the outputs of (b) and (c) are compared bit for bit.  Staging runs inside the
tile kernel's epilogue, so events around kernels cannot split compare from staging: (b) - (a) holds staging + the row
copy of the expand pass together, and a finer split is not taken here.
Shapes: 10k self at the 2 % boundary; 100k self at about 1e8 edges; config 4 (50 000 queries x 10 000 references, 2 %).
Legs alternate within a repetition, so that clock and cache state drift hits all of them alike.  On the 10k shape also:
RefineBoundary.fit_from_sketches against engine.dist + fit_dev (same run), with the peak device memory of each.
No threshold is asserted here: the numbers are the record."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="10k,config4,100k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, models, synth
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    res = {"version": lib.ppk_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def boundary(ref, qry, want_edges, rows):
        """a slope-0 core threshold that gives about want_edges edges, from the quantile of a band's distances"""
        nq = qry.n if qry is not None else ref.n
        band = max(64, min(nq, (4_000_000 // max(ref.n, 1)) // 64 * 64))
        lo = (nq // 2) // 64 * 64
        d, _ = engine.dist(ref, qry, kmers, tbl, q_begin=lo, q_end=min(nq, lo + band))
        core = d[:, 0].sort().values
        x = float(core[min(int(want_edges / rows * core.numel()), core.numel() - 1)].item())
        del d, core
        torch.cuda.empty_cache()
        return x

    def run_shape(name, ref, qry, want_frac=None, want_edges=None, dense_ok=True):
        rows = engine.rows_in_band(ref.n, qry.n if qry is not None else 0, 0, qry.n if qry is not None else ref.n)
        want = want_edges if want_edges is not None else want_frac * rows
        x_max = boundary(ref, qry, want, rows)
        kw = dict(slope=0, x_max=x_max, y_max=0.0)
        e, _ = engine.dist_edges(ref, qry, kmers, tbl, **kw)
        m = int(e.shape[0])
        cap = m
        del e
        rec = {"rows": rows, "edges": m, "x_max": x_max, "legs_ms": {}}

        def leg_a():
            return engine.dist_edges(ref, qry, kmers, tbl, cap=cap, **kw)

        def leg_b():
            return engine.dist_edges_rows(ref, qry, kmers, tbl, cap=cap, **kw)

        def leg_c():
            ed, _ = engine.dist_edges(ref, qry, kmers, tbl, cap=cap, **kw)
            return ed, engine.dist_pairs(ref, qry, kmers, tbl, ed)[0]

        dense = None
        if dense_ok:
            dense, _ = engine.dist(ref, qry, kmers, tbl)

        def leg_d():
            return engine.dist(ref, qry, kmers, tbl, out=dense)

        def leg_b2():
            _lib.set_option("edge_rows_fused", 0)
            try:
                return engine.dist_edges_rows(ref, qry, kmers, tbl, cap=cap, **kw)
            finally:
                _lib.set_option("edge_rows_fused", 1)

        legs = [("a_edges", leg_a), ("b_edges_rows", leg_b), ("c_edges_then_pairs", leg_c), ("b_two_step", leg_b2)]
        if dense_ok:
            legs.append(("d_dense", leg_d))
        # warm every leg (scratch, tables, coded copies), and check (b) == (c) on the bits
        eb, rb, _ = leg_b()
        rec["b_kernel"] = lib.ppk_last_kernel_name().decode()
        ec, rc = leg_c()
        rec["b_equals_c"] = bool(torch.equal(eb, ec) and torch.equal(rb.view(torch.int32), rc.view(torch.int32)))
        del eb, rb, ec, rc
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in legs}
        for _ in range(a.reps):
            for k, fn in legs:
                out, ms = event_ms(fn)
                del out
                times[k].append(ms)
        for k, v in times.items():
            rec["legs_ms"][k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        med = {k: rec["legs_ms"][k]["median"] for k in times}
        rec["price_of_rows_ms_b_minus_a"] = round(med["b_edges_rows"] - med["a_edges"], 4)
        rec["saving_c_over_b"] = round(med["c_edges_then_pairs"] / med["b_edges_rows"], 3)
        rec["b_below_c"] = bool(med["b_edges_rows"] < med["c_edges_then_pairs"])
        res["shapes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
        del dense
        torch.cuda.empty_cache()

    shapes = a.shapes.split(",")
    if "10k" in shapes:
        t = synth.make_sketches_device(10_000, kmers, device="cuda:0")
        db = engine.SketchDB(t, 16, 14)
        del t
        run_shape("10k_self_2pct", db, None, want_frac=0.02)
        if not a.no_fit:
          try:
            names = ["g%d" % k for k in range(db.n)]
            fit = {}
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free0, _ = torch.cuda.mem_get_info(0)
            bgmm = models.BGMMModel.fit_from_sketches(db, kmers, tbl, max_components=2, max_samples=100000, seed=42)
            for rep in range(2):          # (the second is the figure)
                def from_sketches():
                    b = models.RefineBoundary()
                    return b, b.fit_from_sketches(db, kmers, tbl, names, bgmm, 0.0, 0.0)
                (b1, _), ms = event_ms(from_sketches)
                fit["fit_from_sketches_ms"] = round(ms, 3)
                fit["fit_passes"] = b1.fit_passes
            free1, _ = torch.cuda.mem_get_info(0)
            fit["device_bytes_taken_from_sketches"] = int(free0 - free1)
            for rep in range(2):
                def with_matrix():
                    d, _ = engine.dist(db, None, kmers, tbl)
                    b = models.RefineBoundary()
                    b.fit_dev(d, names, bgmm, 0.0, 0.0)
                    return b
                b2, ms = event_ms(with_matrix)
                fit["dist_plus_fit_dev_ms"] = round(ms, 3)
            free2, _ = torch.cuda.mem_get_info(0)
            fit["device_bytes_taken_with_matrix"] = int(free0 - free2)
            fit["same_fit"] = bool(float(b1.optimal_x) == float(b2.optimal_x) and float(b1.optimal_y) == float(b2.optimal_y))
            res["fit_10k"] = fit
          except Exception as e:          # (the record says so; the legs above stand)
            res["fit_10k"] = {"error": "%s: %s" % (type(e).__name__, e)}
          print(json.dumps({"fit_10k": res["fit_10k"]}), flush=True)
        db.close()
        torch.cuda.empty_cache()
    if "config4" in shapes:
        t = synth.make_sketches_device(60_000, kmers, device="cuda:0")
        ref, qry = engine.SketchDB(t[:10_000].contiguous(), 16, 14), engine.SketchDB(t[10_000:].contiguous(), 16, 14)
        del t
        run_shape("config4_50k_x_10k_2pct", ref, qry, want_frac=0.02)
        ref.close()
        qry.close()
        torch.cuda.empty_cache()
    if "100k" in shapes:
        t = synth.make_sketches_device(100_000, kmers, device="cuda:0")
        db = engine.SketchDB(t, 16, 14)
        del t
        torch.cuda.empty_cache()
        run_shape("100k_self_1e8_edges", db, None, want_edges=1e8, dense_ok=False)
        db.close()

    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
