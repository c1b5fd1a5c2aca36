"""Sketching assemblies on the MI355X: FASTA files -> codes -> the bit-sliced bin sketches the distance engine reads
(include/ppk.h "Sketching").

[EXT] The sketch rule -- hash, bin, densify -- is this project's own ("poppunk_amd:sketch1").  pp-sketchlib is not part
of this tree and no assembly with a known upstream sketch is, so sketches made here are NOT bit-compatible with
databases pp-sketchlib wrote: never mix the two in one query.  Databases written from here say so in their
`sketch_version` attribute.

Codes: 0-3 = A, C, G, T (either case); 4 = any other residue (N, IUPAC codes); 5 = contig break, put between the
records of a file and between the files of a sample, so that no k-mer spans two contigs.
"""
import ctypes as C
import gzip
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

SKETCH_VERSION = "poppunk_amd:sketch1"
BBITS = 14
MAX_READ_THREADS = 16

_TABLE = bytearray([4] * 256)
for _code, _letters in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    for _ch in _letters:
        _TABLE[_ch] = _code
_TABLE = bytes(_TABLE)
_DROP = b" \t\r\n"

# where the last sketch_files / sketch_to_db call spent its time, in ms: read (files -> codes, all threads), upload
# (sketch_to_db only: codes to the device), sketch (the engine call: for sketch_files upload, kernels and download)
last_timing = {}


def read_fasta(path):
    """The codes of one FASTA file, uint8: plain or gzip (told by its first two bytes), any number of records with a
    code 5 between them, LF or CRLF line ends, a final newline or none, either case.  An empty file, a FASTQ file
    (read input is not built) and anything else that does not start with '>' raise ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    head = data.lstrip()[:1]
    if not head:
        raise ValueError("%s is empty" % path)
    if head == b"@":
        raise ValueError("%s looks like FASTQ: sketching reads is not built, only assemblies in FASTA" % path)
    if head != b">":
        raise ValueError("%s is not FASTA: it does not start with '>'" % path)
    parts = []
    for record in re.split(rb"(?m)^>", data.lstrip())[1:]:       # a record starts at a '>' that starts a line
        _, _, seq = record.partition(b"\n")
        if parts:
            parts.append(b"\x05")
        parts.append(seq.translate(_TABLE, _DROP))
    return np.frombuffer(b"".join(parts), dtype=np.uint8)


def read_sample(files):
    """One sample's files (a path or a list of paths) as one code array, a code 5 between files."""
    if isinstance(files, (str, bytes)):
        files = [files]
    arrays = []
    for path in files:
        if arrays:
            arrays.append(np.array([5], dtype=np.uint8))
        arrays.append(read_fasta(path))
    return arrays[0] if len(arrays) == 1 else np.concatenate(arrays)


def read_samples(files, threads=1):
    """(codes uint8, seq_off int64 [n + 1]) of every sample, read on at most `threads` host threads (never more than
    16: the work is file reading and a byte translation, both outside the interpreter lock)."""
    workers = max(1, min(int(threads), MAX_READ_THREADS, len(files) or 1))
    if workers == 1:
        per = [read_sample(f) for f in files]
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            per = list(pool.map(read_sample, files))
    seq_off = np.zeros(len(per) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in per], out=seq_off[1:])
    codes = np.concatenate(per) if per else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(codes, dtype=np.uint8), seq_off


def sketchsize64_of(sketch_size):
    s64 = int(sketch_size) // 64
    if s64 < 1:
        raise ValueError("sketch_size must be at least 64 (sketchsize64 = sketch_size // 64 >= 1)")
    return s64


def check_filled(filled, names, klist):
    """Raises, naming them, when a sample has no k-mer at one of the lengths (its words are all zero)."""
    filled = np.asarray(filled)
    bad = np.flatnonzero((filled == 0).any(axis=1)) if filled.size else []
    if len(bad):
        who = ["%s (k = %s)" % (names[i] if names is not None else "sample %d" % i,
                                ",".join(str(int(klist[j])) for j in np.flatnonzero(filled[i] == 0))) for i in bad[:10]]
        raise RuntimeError("no valid k-mer to sketch in %d sample(s): %s%s"
                           % (len(bad), "; ".join(who), " ..." if len(bad) > 10 else ""))


def sketch_codes(codes, seq_off, klist, sketch_size, strand_preserved=False, device_id=0, names=None):
    """Host arrays in, host arrays out (ppk_sketch): codes uint8, seq_off the n + 1 offsets of the samples in it.
    Returns (sketches uint64 [n, nk, sketchsize64 * 14], stats int64 [n, 6] = length, missing bases, A, C, G, T
    counts, filled int32 [n, nk]).  A sample without a single valid k-mer at one of the lengths raises RuntimeError
    naming it (`names`, or its index)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
    if seq_off.ndim != 1 or seq_off.size < 1:
        raise ValueError("seq_off must be a one-dimensional array of n + 1 offsets")
    if seq_off.size > 1 and int(seq_off.max()) > codes.size:
        raise ValueError("seq_off ends beyond codes")
    k = np.ascontiguousarray(klist, dtype=np.int32).ravel()
    s64 = sketchsize64_of(sketch_size)
    n, nk = seq_off.size - 1, int(k.size)
    sketches = np.zeros((n, nk, s64 * BBITS), dtype=np.uint64)
    stats = np.zeros((n, 6), dtype=np.int64)
    filled = np.zeros((n, nk), dtype=np.int32)
    keep = codes if codes.size else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().ppk_sketch(keep.ctypes.data_as(C.POINTER(C.c_uint8)), seq_off.ctypes.data_as(C.POINTER(C.c_longlong)),
                               n, k.ctypes.data_as(C.POINTER(C.c_int32)), nk, s64, BBITS,
                               _lib.SKETCH_STRAND_PRESERVED if strand_preserved else 0, int(device_id),
                               sketches.ctypes.data_as(C.POINTER(C.c_uint64)),
                               stats.ctypes.data_as(C.POINTER(C.c_longlong)),
                               filled.ctypes.data_as(C.POINTER(C.c_int32)))
    _lib.check(rc, "ppk_sketch")
    check_filled(filled, names, k)
    return sketches, stats, filled


def sketch_files(names, files, klist, sketch_size, strand_preserved=False, device_id=0, threads=1):
    """The samples `names`, each from its FASTA file(s) `files[i]` (a path or a list of paths), sketched on device_id.
    Returns what sketch_codes returns."""
    if len(names) != len(files):
        raise ValueError("names and files differ in length")
    last_timing.clear()
    t0 = time.perf_counter()
    codes, seq_off = read_samples(files, threads)
    t1 = time.perf_counter()
    out = sketch_codes(codes, seq_off, klist, sketch_size, strand_preserved, device_id, names=list(names))
    last_timing.update(read=(t1 - t0) * 1e3, sketch=(time.perf_counter() - t1) * 1e3, codes=int(codes.size))
    return out


def sketch_to_db(names, files, klist, sketch_size, strand_preserved=False, device_id=0, threads=1):
    """The same samples as a resident engine.SketchDB: the sketches never visit the host.  Returns (db, stats int64
    [n, 6], filled int32 [n, nk]) with the two small arrays on the host."""
    import torch
    from . import engine
    if len(names) != len(files):
        raise ValueError("names and files differ in length")
    last_timing.clear()
    t0 = time.perf_counter()
    codes, seq_off = read_samples(files, threads)
    t1 = time.perf_counter()
    s64 = sketchsize64_of(sketch_size)
    dev = torch.device("cuda:%d" % int(device_id))
    codes_t = torch.as_tensor(codes if codes.size else np.zeros(1, dtype=np.uint8), device=dev)
    torch.cuda.current_stream(dev).synchronize()
    t2 = time.perf_counter()
    sk, stats, filled = engine.sketch_dev(codes_t, seq_off, klist, s64, BBITS, strand_preserved)
    stats, filled = stats.cpu().numpy(), filled.cpu().numpy()
    check_filled(filled, list(names), np.asarray(klist).ravel())
    db = engine.SketchDB(sk, s64, BBITS, device=int(device_id))
    last_timing.update(read=(t1 - t0) * 1e3, upload=(t2 - t1) * 1e3, sketch=(time.perf_counter() - t2) * 1e3,
                       codes=int(codes.size))
    return db, stats, filled


def base_freq_of(stats):
    """float64 [n, 4]: the A, C, G, T shares of the counted bases (0.25 each for a sample without any)."""
    counts = np.asarray(stats, dtype=np.float64)[:, 2:6]
    total = counts.sum(axis=1, keepdims=True)
    return np.where(total > 0, counts / np.where(total > 0, total, 1.0), 0.25)
