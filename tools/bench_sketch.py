"""Sketching on the MI355X (ppk_sketch_dev): synthetic random genomes of 2 Mbp at k = 13 ... 29 step 4
and sketch size 9 984, generated on the device so that the kernel part reads no files.

    timeout -k 10 600 python tools/bench_sketch.py [--out profiles/sketch/bench_sketch.json]

Records, HIP-event ms per call (median of --steps after two warm-ups; every call holds its own read-back):
  device     engine.sketch_dev on --genomes genomes: per call, per genome, per k-mer hashed, with the library's stage
             split (plan + stats, hash = rolling hashes and per-bin minima, finish = densify + bit-slice)
  pure_read  a pure read of the same code bytes in the same run (torch.sum)
  mixed      the same call with one genome ten times as long as the others next to many short ones
  files      the host-inclusive sketching.sketch_to_db on --file-genomes FASTA files written to a local temporary
             directory: read (files -> codes), upload, kernel
No threshold is asserted here: the numbers are the record.  Not measured here: other sketch sizes, more than one GPU,
gzip input, hardware counters."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_network import stage_table      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--sketch-size", type=int, default=9984)
    ap.add_argument("--file-genomes", type=int, default=8)
    a = ap.parse_args()
    import torch
    from poppunk_amd import _lib, engine, sketching
    lib = _lib.lib()
    kmers = list(range(13, 30, 4))
    s64 = a.sketch_size // 64
    res = {"version": lib.ppk_version().decode(), "steps": a.steps, "kmers": kmers, "sketchsize64": s64,
           "options": {k: _lib.get_option(k) for k in ("sketch_lds_bins", "sketch_batch_mb", "sketch_batch")},
           "cpus": len(os.sched_getaffinity(0))}

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
        return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}

    def stages(fn):
        lib.ppk_prof_stages_enable(1)
        stage_table(lib)
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        lib.ppk_prof_stages_enable(0)
        return {k: round(v["ms"] / a.steps, 4) for k, v in stage_table(lib).items()}

    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261020)

    def run(name, lengths):
        off = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(lengths, out=off[1:])
        codes = torch.randint(0, 4, (int(off[-1]),), generator=g, device="cuda:0", dtype=torch.uint8)
        off_t = torch.as_tensor(off, device="cuda:0")
        call = lambda: engine.sketch_dev(codes, off_t, kmers, s64)
        r = {"genomes": len(lengths), "codes": int(off[-1]), "longest": int(max(lengths)), "call": timed(call),
             "stages_ms_per_call": stages(call),
             "pure_read_of_the_codes": timed(lambda: torch.sum(codes, dtype=torch.int64))}
        hashed = sum(max(0, n - k + 1) for n in lengths for k in kmers)
        r["ms_per_genome"] = round(r["call"]["median_ms"] / len(lengths), 4)
        r["ns_per_kmer_hashed"] = round(r["call"]["median_ms"] * 1e6 / hashed, 5)
        r["over_pure_read"] = round(r["call"]["median_ms"] / r["pure_read_of_the_codes"]["median_ms"], 1)
        res[name] = r
        print(name, json.dumps(r), flush=True)

    run("device", [a.length] * a.genomes)
    run("mixed", [10 * a.length] + [a.length // 100] * (4 * a.genomes))

    # host-inclusive: FASTA files on local disk -> a resident SketchDB
    work = tempfile.mkdtemp(prefix="ppk_bench_sketch_")
    rng = np.random.Generator(np.random.PCG64(3))
    names, files = [], []
    for i in range(a.file_genomes):
        text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=a.length)].tobytes()
        path = os.path.join(work, "g%03d.fa" % i)
        with open(path, "wb") as f:
            f.write(b">g%d\n" % i)
            for at in range(0, len(text), 80):
                f.write(text[at:at + 80] + b"\n")
        names.append("g%03d" % i)
        files.append(path)
    rows = []
    for threads in (1, 8, 16):
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            db, _, _ = sketching.sketch_to_db(names, files, kmers, a.sketch_size, threads=threads)
            wall = (time.perf_counter() - t0) * 1e3
            db.close()
            if best is None or wall < best["wall_ms"]:
                best = dict(threads=threads, wall_ms=round(wall, 2),
                            **{k: round(v, 2) for k, v in sketching.last_timing.items() if k != "codes"})
        rows.append(best)
    res["files"] = {"genomes": a.file_genomes, "length": a.length, "best_of_3": rows,
                    "note": "sketch = device call, SketchDB re-layout and the two small downloads"}
    print("files", json.dumps(res["files"]), flush=True)
    for path in files:
        os.remove(path)
    os.rmdir(work)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
