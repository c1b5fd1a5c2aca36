"""Sketching read sets on the MI355X (ppk_sketch_reads_dev): simulated reads of random 2 Mbp genomes at
50x (100-base reads, 1 % substitutions, half of them reverse-complemented), generated on the device, at k = 13 ... 29
step 4 and sketch size 9 984, min_count 3.

    timeout -k 10 900 python tools/bench_sketch_reads.py [--out profiles/sketch_reads/bench_sketch_reads.json]

Records, from ONE run, HIP-event ms per call (median of --steps after one warm-up; every call holds its own read-backs):
  table / exact   engine.sketch_reads_dev on --samples read sets, with the library's stage split (plan + stats, count,
                  select, winners, finish; the exact route's rounds add to select and winners)
  single_pass     engine.sketch_dev, the assembly route's one hash pass, over the same codes
  pure_read       a pure read of the same code bytes (torch.sum)
and the ratios of the read calls to the single pass.  No threshold is asserted here: the numbers are the record.  Not
measured here: real reads, other coverages, error rates, sketch sizes or min_count, forced table sizes, more than one
GPU, hardware counters, FASTQ parsing on the host."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--coverage", type=float, default=50.0)
    ap.add_argument("--sketch-size", type=int, default=9984)
    ap.add_argument("--min-count", type=int, default=3)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    kmers = list(range(13, 30, 4))
    s64 = a.sketch_size // 64
    res = {"version": lib.ppk_version().decode(), "steps": a.steps, "kmers": kmers, "sketchsize64": s64,
           "min_count": a.min_count, "samples": a.samples, "genome_length": a.length, "coverage": a.coverage,
           "options": {k: _lib.get_option(k) for k in ("sketch_lds_bins", "sketch_count_bits", "sketch_exact_rounds")}}

    g = torch.Generator(device=dev)
    g.manual_seed(20261020)
    read_len, n_reads = 100, int(round(a.coverage * a.length / 100))
    parts = []
    for _ in range(a.samples):
        genome = torch.randint(0, 4, (a.length,), generator=g, device=dev, dtype=torch.uint8)
        starts = torch.randint(0, a.length, (n_reads, 1), generator=g, device=dev)
        reads = genome[(starts + torch.arange(read_len, device=dev)[None, :]) % a.length]
        hit = torch.rand(reads.shape, generator=g, device=dev) < 0.01
        reads = torch.where(hit, (reads + torch.randint(1, 4, reads.shape, generator=g, device=dev, dtype=torch.uint8)) % 4, reads)
        flip = torch.rand((n_reads, 1), generator=g, device=dev) < 0.5
        reads = torch.where(flip, 3 - reads.flip(1), reads)
        parts.append(torch.cat([reads, torch.full((n_reads, 1), 5, device=dev, dtype=torch.uint8)], dim=1).reshape(-1))
        del genome, starts, hit, flip, reads
    off = np.zeros(a.samples + 1, dtype=np.int64)
    np.cumsum([int(p.numel()) for p in parts], out=off[1:])
    codes = torch.cat(parts)
    del parts
    off_t = torch.as_tensor(off, device=dev)
    res["codes"] = int(off[-1])
    res["count_bits"] = [min(26, max(12, int(np.ceil(np.log2(int(n)))) + 2)) for n in np.diff(off)]      # ppk_sketch_count_bits

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}

    def stages(fn):
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        fn()
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        return {k: {"ms": round(v["ms"], 3), "count": v["count"]} for k, v in stage_table(lib).items()}

    calls = {"table": lambda: engine.sketch_reads_dev(codes, off_t, kmers, s64, a.min_count, False),
             "exact": lambda: engine.sketch_reads_dev(codes, off_t, kmers, s64, a.min_count, True),
             "single_pass": lambda: engine.sketch_dev(codes, off_t, kmers, s64),
             "pure_read": lambda: torch.sum(codes, dtype=torch.int64)}
    for name, call in calls.items():
        r = {"call": timed(call)}
        if name != "pure_read":
            r["stages_of_one_call"] = stages(call)
        res[name] = r
        print(name, json.dumps(r), flush=True)
    kst = calls["table"]()[3].cpu().numpy()
    res["kstats_of_sample_0"] = kst[0].tolist()
    res["lengths"] = calls["table"]()[1][:, 0].cpu().numpy().tolist()
    single = res["single_pass"]["call"]["median_ms"]
    res["table_over_single_pass"] = round(res["table"]["call"]["median_ms"] / single, 2)
    res["exact_over_single_pass"] = round(res["exact"]["call"]["median_ms"] / single, 2)
    res["single_pass_over_pure_read"] = round(single / res["pure_read"]["call"]["median_ms"], 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
