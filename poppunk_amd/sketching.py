"""Sketching assemblies and read sets on the MI355X: FASTA / FASTQ files -> codes -> the bit-sliced bin sketches the
distance engine reads (include/ppk.h "Sketching" and "Sketching read sets").

[EXT] The sketch rule -- hash, bin, densify -- is this project's own ("poppunk_amd:sketch1").  pp-sketchlib is not part
of this tree and no assembly with a known upstream sketch is, so sketches made here are NOT bit-compatible with
databases pp-sketchlib wrote: never mix the two in one query.  Databases written from here say so in their
`sketch_version` attribute.

Codes: 0-3 = A, C, G, T (either case); 4 = any other residue (N, IUPAC codes); 5 = contig break, put between the
records of a file and between the files of a sample, so that no k-mer spans two contigs.  Every read of a FASTQ file
is a contig.

Read sets: a sample whose files are FASTQ is sketched with the same rule, but a k-mer may enter a
bin only when the sample holds it at least `min_count` times ([EXT] the count table's rows, remix and default size
are this project's own; `exact=True` counts the winners exactly).  Its stored `length` is an estimate of its distinct
admitted k-mers, not its number of read bases.
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
_TABLE_READS = bytearray(_TABLE)      # reads are joined by a newline, which becomes the contig break
_TABLE_READS[0x0a] = 5
_TABLE_READS = bytes(_TABLE_READS)
_DROP = b" \t\r\n"

# where the last sketch_files / sketch_to_db call spent its time, in ms: read (files -> codes, all threads), upload
# (sketch_to_db only: codes to the device), sketch (the engine call: for sketch_files upload, kernels and download)
last_timing = {}


def _file_bytes(path):
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


def _fasta_codes(path, data):
    head = data.lstrip()[:1]
    if not head:
        raise ValueError("%s is empty" % path)
    if head == b"@":
        raise ValueError("%s looks like FASTQ: reads are sketched with a minimum k-mer count of 1 or more "
                         "(min_count), not as an assembly" % path)
    if head != b">":
        raise ValueError("%s is not FASTA: it does not start with '>'" % path)
    parts = []
    for record in re.split(rb"(?m)^>", data.lstrip())[1:]:       # a record starts at a '>' that starts a line
        _, _, seq = record.partition(b"\n")
        if parts:
            parts.append(b"\x05")
        parts.append(seq.translate(_TABLE, _DROP))
    return np.frombuffer(b"".join(parts), dtype=np.uint8)


def read_fasta(path):
    """The codes of one FASTA file, uint8: plain or gzip (told by its first two bytes), any number of records with a
    code 5 between them, LF or CRLF line ends, a final newline or none, either case.  An empty file, a FASTQ file
    (reads are not assemblies: read_fastq and a min_count are for them) and anything else that does not start with
    '>' raise ValueError."""
    return _fasta_codes(path, _file_bytes(path))


def _fastq_codes(path, data):
    lines = data.replace(b"\r\n", b"\n").lstrip().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                     # (the final newline)
    if len(lines) % 4 == 3 and lines[-1][:1] == b"+" and lines[-2] == b"":
        lines.append(b"")                               # (an empty last read whose empty quality line has no newline)
    if not lines:
        raise ValueError("%s is empty" % path)
    heads, seqs, plus, quals = lines[0::4], lines[1::4], lines[2::4], lines[3::4]
    for i, (h, s, p, q) in enumerate(zip(heads, seqs, plus, quals)):      # (the whole records; the first fault is named)
        if h[:1] != b"@" or p[:1] != b"+":
            raise ValueError("%s: record %d is not a four-line FASTQ record ('@' and '+' lines expected)" % (path, i + 1))
        if len(s) != len(q):
            raise ValueError("%s: record %d has %d bases and %d qualities" % (path, i + 1, len(s), len(q)))
    if len(lines) % 4:
        raise ValueError("%s: record %d is truncated (a FASTQ record has four lines)" % (path, len(lines) // 4 + 1))
    return np.frombuffer(b"\n".join(seqs).translate(_TABLE_READS, b" \t\r"), dtype=np.uint8)


def read_fastq(path):
    """The codes of one FASTQ file, uint8: plain or gzip, four-line records (name, sequence, '+' with or without the
    name, qualities) read BY RECORD -- a quality line may begin with '@' -- with LF or CRLF line ends, a final newline
    or none, either case; an empty read is allowed.  A code 5 stands between reads; qualities are ignored.  Multi-line
    FASTQ (a sequence wrapped over several lines) is NOT read.  A truncated record, or a sequence and quality of
    different lengths, raises a one-line ValueError naming the file and the record."""
    data = _file_bytes(path)
    head = data.lstrip()[:1]
    if not head:
        raise ValueError("%s is empty" % path)
    if head != b"@":
        raise ValueError("%s is not FASTQ: it does not start with '@'" % path)
    return _fastq_codes(path, data)


def read_sequence_file(path):
    """(codes, is_reads) of a FASTA or FASTQ file, told apart by its first byte ('>' or '@')."""
    data = _file_bytes(path)
    if data.lstrip()[:1] == b"@":
        return _fastq_codes(path, data), True
    return _fasta_codes(path, data), False


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


def read_sample_kind(files):
    """(codes, is_reads) of one sample's files, FASTA or FASTQ: a sample is reads when its files are FASTQ; both
    kinds within one sample raise ValueError."""
    if isinstance(files, (str, bytes)):
        files = [files]
    arrays, kinds = [], set()
    for path in files:
        if arrays:
            arrays.append(np.array([5], dtype=np.uint8))
        codes, is_reads = read_sequence_file(path)
        arrays.append(codes)
        kinds.add(is_reads)
    if len(kinds) > 1:
        raise ValueError("FASTA and FASTQ files within one sample: %s" % ", ".join(str(f) for f in files))
    return (arrays[0] if len(arrays) == 1 else np.concatenate(arrays)), kinds.pop()


def _read_all(files, threads):
    """(per-sample code arrays, reads flags bool [n]) on at most `threads` host threads (16 at the most)"""
    workers = max(1, min(int(threads), MAX_READ_THREADS, len(files) or 1))
    if workers == 1:
        per = [read_sample_kind(f) for f in files]
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            per = list(pool.map(read_sample_kind, files))
    return [a for a, _ in per], np.array([r for _, r in per], dtype=bool)


def _joined(arrays):
    seq_off = np.zeros(len(arrays) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in arrays], out=seq_off[1:])
    codes = np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(codes, dtype=np.uint8), seq_off


def check_min_count(reads, names, min_count, exact):
    """The rule of the surface, before any device call: read samples need min_count >= 1 (ValueError); min_count or
    exact without a read sample is an error too (RuntimeError).  Returns min_count as an int (0 without reads)."""
    mc = 0 if min_count is None else int(min_count)
    reads = np.asarray(reads, dtype=bool)
    if reads.any() and mc < 1:
        who = [str(names[i]) for i in np.flatnonzero(reads)[:5]]
        raise ValueError("%s looks like FASTQ: give a minimum k-mer count of 1 or more (min_count) to sketch reads"
                         % ", ".join(who))
    if not reads.any() and (mc >= 1 or exact):
        raise RuntimeError("min_count and exact apply to read samples (FASTQ) and none was given")
    return mc


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


def sketch_read_codes(codes, seq_off, klist, sketch_size, min_count, exact=False, strand_preserved=False, device_id=0,
                      names=None):
    """Read samples, host arrays in, host arrays out (ppk_sketch_reads): as sketch_codes, with a k-mer
    entering a bin only when the sample holds it at least min_count times (1 .. 65 535; exact: the exact route).
    Returns (sketches, stats, filled, kstats int64 [n, nk, 4] = occ, adm_occ, filled, win_occ); stats[:, 0] is the
    estimate of the distinct admitted k-mers at the largest k, not the number of read bases.  A sample without an
    admitted k-mer at one of the lengths raises RuntimeError naming it."""
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
    kstats = np.zeros((n, nk, 4), dtype=np.int64)
    filled = np.zeros((n, nk), dtype=np.int32)
    keep = codes if codes.size else np.zeros(1, dtype=np.uint8)
    flags = (_lib.SKETCH_STRAND_PRESERVED if strand_preserved else 0) | (_lib.SKETCH_EXACT if exact else 0)
    rc = _lib.lib().ppk_sketch_reads(keep.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     seq_off.ctypes.data_as(C.POINTER(C.c_longlong)), n,
                                     k.ctypes.data_as(C.POINTER(C.c_int32)), nk, s64, BBITS, flags, int(min_count),
                                     int(device_id), sketches.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     stats.ctypes.data_as(C.POINTER(C.c_longlong)),
                                     kstats.ctypes.data_as(C.POINTER(C.c_longlong)),
                                     filled.ctypes.data_as(C.POINTER(C.c_int32)))
    _lib.check(rc, "ppk_sketch_reads")
    check_filled(filled, names, k)
    return sketches, stats, filled, kstats


# whether each sample of the last sketch_files / sketch_to_db call was reads (bool [n])
last_reads = np.zeros(0, dtype=bool)


def _read_and_split(names, files, threads, min_count, exact):
    """(min_count, reads flags, [(sample indices, codes, seq_off, is_reads) per kind present]) of a batch"""
    global last_reads
    if len(names) != len(files):
        raise ValueError("names and files differ in length")
    arrays, reads = _read_all(files, threads)
    mc = check_min_count(reads, names, min_count, exact)
    last_reads = reads
    parts = []
    for kind in (False, True):
        idx = np.flatnonzero(reads == kind)
        if idx.size:
            parts.append((idx,) + _joined([arrays[i] for i in idx]) + (kind,))
    return mc, reads, parts


def sketch_files(names, files, klist, sketch_size, strand_preserved=False, device_id=0, threads=1, min_count=0,
                 exact=False):
    """The samples `names`, each from its file(s) `files[i]` (a path or a list of paths; FASTA = an assembly, FASTQ =
    reads), sketched on device_id: the assemblies in one ppk_sketch call, the read samples in one ppk_sketch_reads
    call with `min_count` / `exact`, rows in the caller's order.  Returns what sketch_codes returns; `last_reads` says
    which samples were reads.  Reads need min_count >= 1; min_count or exact without reads is an error."""
    last_timing.clear()
    t0 = time.perf_counter()
    mc, reads, parts = _read_and_split(names, files, threads, min_count, exact)
    t1 = time.perf_counter()
    k = np.asarray(klist).ravel()
    n, s64 = len(names), sketchsize64_of(sketch_size)
    sketches = np.zeros((n, k.size, s64 * BBITS), dtype=np.uint64)
    stats = np.zeros((n, 6), dtype=np.int64)
    filled = np.zeros((n, k.size), dtype=np.int32)
    for idx, codes, seq_off, is_reads in parts:
        sub = [names[i] for i in idx]
        if is_reads:
            out = sketch_read_codes(codes, seq_off, klist, sketch_size, mc, exact, strand_preserved, device_id, names=sub)
        else:
            out = sketch_codes(codes, seq_off, klist, sketch_size, strand_preserved, device_id, names=sub)
        sketches[idx], stats[idx], filled[idx] = out[0], out[1], out[2]
    last_timing.update(read=(t1 - t0) * 1e3, sketch=(time.perf_counter() - t1) * 1e3,
                       codes=int(sum(p[1].size for p in parts)))
    return sketches, stats, filled


def sketch_to_db(names, files, klist, sketch_size, strand_preserved=False, device_id=0, threads=1, min_count=0,
                 exact=False):
    """The same samples as a resident engine.SketchDB: the sketches never visit the host.  Returns (db, stats int64
    [n, 6], filled int32 [n, nk]) with the two small arrays on the host.  min_count / exact as sketch_files."""
    import torch
    from . import engine
    last_timing.clear()
    t0 = time.perf_counter()
    mc, reads, parts = _read_and_split(names, files, threads, min_count, exact)
    t1 = time.perf_counter()
    s64 = sketchsize64_of(sketch_size)
    dev = torch.device("cuda:%d" % int(device_id))
    tensors = [torch.as_tensor(codes if codes.size else np.zeros(1, dtype=np.uint8), device=dev) for _, codes, _, _ in parts]
    torch.cuda.current_stream(dev).synchronize()
    t2 = time.perf_counter()
    n, nk = len(names), int(np.asarray(klist).size)
    sk = torch.zeros((n, nk, s64 * BBITS), dtype=torch.int64, device=dev) if len(parts) != 1 else None
    stats = np.zeros((n, 6), dtype=np.int64)
    filled = np.zeros((n, nk), dtype=np.int32)
    for (idx, _, seq_off, is_reads), codes_t in zip(parts, tensors):
        if is_reads:
            out = engine.sketch_reads_dev(codes_t, seq_off, klist, s64, mc, exact, BBITS, strand_preserved)
        else:
            out = engine.sketch_dev(codes_t, seq_off, klist, s64, BBITS, strand_preserved)
        if sk is None:
            sk = out[0]
        else:
            sk[torch.as_tensor(idx, device=dev)] = out[0]
        stats[idx], filled[idx] = out[1].cpu().numpy(), out[2].cpu().numpy()
    check_filled(filled, list(names), np.asarray(klist).ravel())
    db = engine.SketchDB(sk, s64, BBITS, device=int(device_id))
    last_timing.update(read=(t1 - t0) * 1e3, upload=(t2 - t1) * 1e3, sketch=(time.perf_counter() - t2) * 1e3,
                       codes=int(sum(p[1].size for p in parts)))
    return db, stats, filled


def base_freq_of(stats):
    """float64 [n, 4]: the A, C, G, T shares of the counted bases (0.25 each for a sample without any)."""
    counts = np.asarray(stats, dtype=np.float64)[:, 2:6]
    total = counts.sum(axis=1, keepdims=True)
    return np.where(total > 0, counts / np.where(total > 0, total, 1.0), 0.25)
