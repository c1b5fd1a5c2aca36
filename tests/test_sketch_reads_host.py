"""CPU tests of sketching read sets, no GPU: the numpy restatement of the rule
(tests/sketch_reads_model.py) against hand values and against its own claims -- the count filter recovers the
assembly's sketch from reads, the table route equals the exact route at the default size, the length estimate is
within its standard error -- the ppk_device.h functions run on the host against the model
(sketch_reads_device_host.hip), read_fastq, the surface of sketch_files / constructDatabase, the `reads` flag of the
database writers and the argument errors of the C ABI.

[EXT] The count table (rows, remix, default bits) is this project's own: these are checks of the reference the GPU
tests compare the kernels with, not of upstream parity."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import sketch_model as sm
import sketch_reads_model as rm
from poppunk_amd import _lib, pp_sketchlib, sketchdb, sketching

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = (1 << 64) - 1


# ---- the model against hand values -------------------------------------------------------------------------------

def test_row_index_and_default_bits_by_hand():
    for h in (0, 1, 0x123456789abcdef0, M64 - 1):
        for row, mult in ((0, 0x9e3779b97f4a7c15), (1, 0xc2b2ae3d27d4eb4f)):
            for bits in (4, 12, 22, 26):
                want = (((h ^ (h >> 29)) * mult) & M64) >> (64 - bits)
                assert int(rm.count_index(np.array([h], dtype=np.uint64), row, bits)[0]) == want
    assert [rm.count_bits(n) for n in (0, 1, 1024, 1025, 4039, 605_999, 1 << 24, (1 << 24) + 1, 10 ** 8, 1 << 40)] == \
        [12, 12, 12, 13, 14, 22, 26, 26, 26, 26]
    assert rm.length_estimate(0, 0, 0) == 0 and rm.length_estimate(10, 0, 0) == 0
    assert rm.length_estimate(100, 4, 8) == 50 and rm.length_estimate(3, 1, 2) == 2 and rm.length_estimate(5, 1, 4) == 1


def test_counts_and_admission_by_hand():
    # ACGTA three times, CCCCC twice, GGTGG once, as separate reads: k = 5, one k-mer each (both strands count together)
    reads = [[0, 1, 2, 3, 0]] * 2 + [[1, 1, 1, 1, 1]] * 2 + [[2, 2, 3, 2, 2]] + [[3, 0, 1, 2, 3]]      # TACGT = rc(ACGTA)
    codes = np.concatenate([np.array(r + [5], dtype=np.uint8) for r in reads])[:-1]
    h = rm.kept_hashes(codes, 5)
    assert len(h) == 6 and rm.exact_counts(h).tolist() == [3, 3, 2, 2, 1, 3]
    assert rm.exact_counts(rm.kept_hashes(codes, 5, strand_preserved=True)).tolist() == [2, 2, 2, 2, 1, 1]
    for min_count, admitted in ((1, 6), (2, 5), (3, 3), (4, 0)):
        for exact in (False, True):
            m, kstats = rm.admitted_minima(h, 64, min_count, exact, 20)
            assert kstats.tolist()[:2] == [6, admitted]
            want = np.unique(h[rm.exact_counts(h) >= min_count])
            assert sorted(m[m != sm.EMPTY].tolist()) == sorted(want.tolist()) and kstats[2] == len(want)
            assert kstats[3] == admitted                       # (every admitted k-mer is alone in its bin here)
    # a table of 2^4 counters: what it admits is a superset of the exact route's, and the exact route ignores it
    rng = np.random.Generator(np.random.PCG64(3))
    codes = rm.simulate_reads(rng, sm.random_genome(rng, 400), 6, read_len=50)[0]
    h = rm.kept_hashes(codes, 13)
    loose = rm.table_admits(h, 3, 4)
    assert loose.all() and not (rm.exact_counts(h) >= 3).all()
    assert np.array_equal(rm.admitted_minima(h, 64, 3, True, 4)[0], rm.admitted_minima(h, 64, 3, True, 24)[0])
    assert not np.array_equal(rm.admitted_minima(h, 64, 3, False, 4)[0], rm.admitted_minima(h, 64, 3, True, 4)[0])


def test_simulated_reads_have_the_stated_shape():
    rng = np.random.Generator(np.random.PCG64(8))
    g = sm.random_genome(rng, 5000)
    codes, n_reads = rm.simulate_reads(rng, g, 20)
    assert n_reads == 1000 and len(codes) == 1000 * 101 - 1
    reads = np.append(codes, np.uint8(5)).reshape(1000, 101)
    assert (reads[:, 100] == 5).all() and (reads[:, :100] < 5).all()
    assert 5 <= (reads == 4).any(axis=1).sum() <= 45          # 2 % of the reads carry one N
    both = np.concatenate([g, g[:99]])
    windows = {bytes(both[i:i + 100]) for i in range(5000)}
    rc = {bytes(sm.reverse_complement(np.frombuffer(w, dtype=np.uint8))) for w in windows}
    clean = [bytes(r[:100]) for r in reads]
    fwd, rev = sum(r in windows for r in clean), sum(r in rc for r in clean)
    assert 100 < fwd < 260 and 100 < rev < 260                # error-free reads (0.99^100 = 0.37 of them), half reversed


# ---- the model's own claims (the issue's figures as conditions) ------------------------------------------------------

@pytest.fixture(scope="module", params=[1, 2, 3])
def read_set(request):
    """a 20 000-base genome at 30x in 100-base reads with 1 % substitutions"""
    rng = np.random.Generator(np.random.PCG64(request.param))
    g = sm.random_genome(rng, 20_000)
    return g, rm.simulate_reads(rng, g, 30)[0]


@pytest.mark.parametrize("k", [13, 21, 29])
def test_the_count_filter_recovers_the_assemblys_sketch(read_set, k):
    g, codes = read_set
    nbins, min_count, bits = 256, 3, rm.count_bits(len(codes))
    assert bits == 22
    assembly = sm.minima(rm.closed_assembly(g, k), k, nbins)
    h = rm.kept_hashes(codes, k)
    exact, _ = rm.admitted_minima(h, nbins, min_count, True, bits)
    table, kstats = rm.admitted_minima(h, nbins, min_count, False, bits)
    raw, _ = rm.admitted_minima(h, nbins, 1, False, bits)
    assert np.array_equal(raw, sm.minima(codes, k, nbins))    # min_count 1 is the plain sketch of the same codes
    share, raw_share = float((exact == assembly).mean()), float((raw == assembly).mean())
    print("k %d: exact route %.3f, unfiltered %.3f of the bins equal the assembly's" % (k, share, raw_share))
    assert share >= 0.98 and raw_share <= 0.50
    assert np.array_equal(table, exact)
    # the length estimate against the number of distinct admitted k-mers, in standard errors cv(winner counts) / sqrt(filled)
    admitted = np.unique(h[rm.table_admits(h, min_count, bits)])
    winners = table[table != sm.EMPTY]
    counts = np.array([int((h == w).sum()) for w in winners])
    assert counts.sum() == kstats[3] and len(winners) == kstats[2]
    se = counts.std() / counts.mean() / np.sqrt(len(winners))
    estimate = rm.length_estimate(kstats[1], kstats[2], kstats[3])
    z = (estimate - len(admitted)) / (se * len(admitted))
    print("k %d: length estimate %d, admitted distinct k-mers %d, z %+.2f" % (k, estimate, len(admitted), z))
    assert abs(z) <= 4.0 and abs(estimate - 20_000) < 2_000


# ---- the device helpers on the host -----------------------------------------------------------------------------------

def test_read_helpers_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    rng = np.random.Generator(np.random.PCG64(21))
    lines = []
    hs = np.concatenate([rng.integers(0, 1 << 63, size=300, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                         np.array([0, 1, 1 << 29, (1 << 63) - 1, 1 << 63, M64 - 1], dtype=np.uint64)])
    for bits in (4, 5, 12, 16, 22, 26):
        for row in range(rm.ROWS):
            for hv, idx in zip(hs.tolist(), rm.count_index(hs, row, bits).tolist()):
                lines.append("I %x %d %d %d" % (hv, row, bits, idx))
    for codes in [0, 1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 605_999, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 10 ** 8,
                  (1 << 32) - 1, 1 << 40, (1 << 62) + 5] + rng.integers(0, 1 << 30, size=50).tolist():
        lines.append("D %d %d" % (codes, rm.count_bits(codes)))
    for adm, filled, win in [(0, 0, 0), (5, 0, 0), (100, 4, 8), (3, 1, 2), (5, 1, 4), ((1 << 43) - 1, (1 << 19) - 1, 1),
                             ((1 << 43) - 1, (1 << 19) - 1, (1 << 43) - 1), (462_280, 255, 6_015)] + \
            [tuple(int(x) for x in rng.integers(1, 1 << 30, size=3) // np.array([1, 1 << 14, 1 << 10]) + 1) for _ in range(50)]:
        lines.append("L %d %d %d %d" % (adm, filled, win, rm.length_estimate(adm, filled, win)))
    for bits, min_count, n in ((4, 3, 40), (6, 2, 100), (10, 3, 3000), (16, 2, 3000)):
        h = rng.integers(0, 1 << 63, size=n // 2, dtype=np.uint64)
        h = np.concatenate([h, h[: n // 4], h[: n // 8], h[: n // 8]])
        lines.append("T %d %d %d %s" % (bits, min_count, len(h), " ".join("%x" % x for x in h.tolist())))
        lines.append("A " + " ".join(str(int(x)) for x in rm.table_admits(h, min_count, bits)))
    records = tmp_path / "records.txt"
    records.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "sketch_reads_device_host")
    # The sanitizers are for the host code alone: -Xarch_host keeps them off any device pass.
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17",
                          "-Xarch_host", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                          os.path.join(HERE, "sketch_reads_device_host.hip"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe, str(records)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert " 0 wrong" in run.stdout
    assert int(run.stdout.split()[0]) == sum(1 for ln in lines if ln[0] in "IDL") + sum(len(ln.split()) - 1 for ln in lines if ln[0] == "A")


# ---- read_fastq ------------------------------------------------------------------------------------------------------

def test_read_fastq_forms(tmp_path):
    want = [0, 1, 2, 3, 4, 5, 3, 3, 5, 5, 2]
    text = "@r1 first\nACGTN\n+r1 first\n@IIII\n@r2\nTT\n+\n@+\n@r3\n\n+\n\n@r4\ng\n+\n@\n"
    forms = {"plain.fq": text.encode(), "crlf.fq": text.replace("\n", "\r\n").encode(),
             "no_final_newline.fq": text[:-1].encode(), "lower.fq": text.lower().encode(),
             "leading_blank.fq": ("\n" + text).encode()}
    for name, data in forms.items():
        (tmp_path / name).write_bytes(data)
        got = sketching.read_fastq(str(tmp_path / name))
        assert got.dtype == np.uint8 and got.tolist() == want, name
        codes, is_reads = sketching.read_sequence_file(str(tmp_path / name))
        assert is_reads and codes.tolist() == want
    with gzip.open(tmp_path / "packed.fq.gz", "wb") as f:
        f.write(text.encode())
    assert sketching.read_fastq(str(tmp_path / "packed.fq.gz")).tolist() == want
    (tmp_path / "empty_last.fq").write_bytes(b"@a\nAC\n+\nII\n@b\n\n+\n")      # an empty last read, no final newline
    assert sketching.read_fastq(str(tmp_path / "empty_last.fq")).tolist() == [0, 1, 5]
    (tmp_path / "one.fq").write_bytes(b"@a\nACGT\n+\n@@@@")
    assert sketching.read_fastq(str(tmp_path / "one.fq")).tolist() == [0, 1, 2, 3]
    (tmp_path / "a.fa").write_bytes(b">a\nAC\n")
    codes, is_reads = sketching.read_sequence_file(str(tmp_path / "a.fa"))
    assert not is_reads and codes.tolist() == [0, 1]
    # a sample of two FASTQ files: a break between them; FASTA and FASTQ within one sample is an error
    codes, is_reads = sketching.read_sample_kind([str(tmp_path / "one.fq"), str(tmp_path / "one.fq")])
    assert is_reads and codes.tolist() == [0, 1, 2, 3, 5, 0, 1, 2, 3]
    with pytest.raises(ValueError, match="FASTA and FASTQ files within one sample") as e:
        sketching.read_sample_kind([str(tmp_path / "one.fq"), str(tmp_path / "a.fa")])
    assert "\n" not in str(e.value)
    assert "Multi-line FASTQ" in " ".join(sketching.read_fastq.__doc__.split())


def test_read_fastq_errors(tmp_path):
    cases = {"truncated.fq": (b"@a\nACGT\n+\nIIII\n@b\nAC\n", r"truncated\.fq: record 2 is truncated"),
             "short_quality.fq": (b"@a\nACGT\n+\nIIII\n@b\nACG\n+\nII\n", r"short_quality\.fq: record 2 has 3 bases and 2 qualities"),
             "multi_line.fq": (b"@a\nACGT\nACGT\n+\nIIIIIIII\n@b\nA\n+\nI\n", r"multi_line\.fq: record 1 is not a four-line"),
             "no_plus.fq": (b"@a\nACGT\nIIII\nIIII\n", r"no_plus\.fq: record 1 is not a four-line"),
             "empty.fq": (b"", r"empty\.fq is empty"), "blank.fq": (b"\n\n", r"blank\.fq is empty"),
             "fasta.fq": (b">a\nACGT\n", r"fasta\.fq is not FASTQ")}
    for name, (data, message) in cases.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError, match=message) as e:
            sketching.read_fastq(str(tmp_path / name))
        assert "\n" not in str(e.value), name
    with pytest.raises(OSError):
        sketching.read_fastq(str(tmp_path / "missing.fq"))
    (tmp_path / "reads.fq").write_bytes(b"@r1\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError, match="looks like FASTQ.*minimum k-mer count of 1 or more"):
        sketching.read_fasta(str(tmp_path / "reads.fq"))          # read_fasta keeps refusing FASTQ


# ---- the surface: errors before any device call, rows in the caller's order ---------------------------------------------

@pytest.fixture
def mixed(tmp_path, monkeypatch):
    """two assemblies and two read samples, and stand-ins for the two engine calls that record what they were given"""
    (tmp_path / "a0.fa").write_bytes(b">a\nACGTACGTAC\n")
    (tmp_path / "a1.fa").write_bytes(b">a\nTTTTTTTT\n>b\nGG\n")
    (tmp_path / "r0.fq").write_bytes(b"@r\nACGT\n+\nIIII\n@s\nGGA\n+\nIII\n")
    with gzip.open(tmp_path / "r1.fq.gz", "wb") as f:
        f.write(b"@r\nCC\n+\nII\n")
    calls = []

    def fake(kind):
        def call(codes, seq_off, klist, sketch_size, *args, **kw):
            calls.append((kind, codes.tolist(), seq_off.tolist(), args, kw))
            n, nk = len(seq_off) - 1, len(klist)
            lengths = np.diff(seq_off)
            stats = np.zeros((n, 6), dtype=np.int64)
            stats[:, 0] = lengths + (1000 if kind == "reads" else 0)
            words = np.zeros((n, nk, 14), dtype=np.uint64) + lengths[:, None, None].astype(np.uint64)
            return (words, stats, np.ones((n, nk), dtype=np.int32)) + ((np.zeros((n, nk, 4), dtype=np.int64),) if kind == "reads" else ())
        return call

    monkeypatch.setattr(sketching, "sketch_codes", fake("assemblies"))
    monkeypatch.setattr(sketching, "sketch_read_codes", fake("reads"))
    names = ["r1", "a0", "r0", "a1"]
    files = [str(tmp_path / "r1.fq.gz"), [str(tmp_path / "a0.fa")], str(tmp_path / "r0.fq"), str(tmp_path / "a1.fa")]
    return dict(names=names, files=files, calls=calls, root=tmp_path)


def test_sketch_files_splits_a_batch_and_keeps_the_callers_order(mixed):
    words, stats, filled = sketching.sketch_files(mixed["names"], mixed["files"], [13, 21], 64, min_count=3, exact=True,
                                                  threads=3)
    assert [c[0] for c in mixed["calls"]] == ["assemblies", "reads"]
    assert mixed["calls"][0][1:3] == ([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 3, 3, 3, 3, 3, 3, 3, 3, 5, 2, 2], [0, 10, 21])
    assert mixed["calls"][1][1:3] == ([1, 1, 0, 1, 2, 3, 5, 2, 2, 0], [0, 2, 10])
    assert mixed["calls"][1][3][:2] == (3, True) and mixed["calls"][1][4]["names"] == ["r1", "r0"]
    assert stats[:, 0].tolist() == [1002, 10, 1008, 11] and words[:, 0, 0].tolist() == [2, 10, 8, 11]
    assert filled.shape == (4, 2) and sketching.last_reads.tolist() == [True, False, True, False]


def test_the_surface_refuses_before_any_device_call(mixed, tmp_path):
    kw = dict(klist=[13, 21], sketch_size=64)
    for min_count in (0, None):
        db = str(tmp_path / "none" / "none")
        with pytest.raises(ValueError, match="looks like FASTQ.*minimum k-mer count of 1 or more") as e:
            pp_sketchlib.constructDatabase(db, mixed["names"], mixed["files"], min_count=min_count, **kw)
        assert "\n" not in str(e.value) and not os.path.exists(db + ".h5") and not os.path.exists(db + ".npz")
    only = [i for i, n in enumerate(mixed["names"]) if n.startswith("a")]
    for extra in (dict(min_count=1), dict(min_count=5), dict(exact=True)):
        with pytest.raises(RuntimeError, match="reads.*none was given") as e:
            pp_sketchlib.constructDatabase(str(tmp_path / "x" / "x"), [mixed["names"][i] for i in only],
                                           [mixed["files"][i] for i in only], **kw, **extra)
        assert "\n" not in str(e.value)
    with pytest.raises(RuntimeError, match="codon_phased"):
        pp_sketchlib.constructDatabase(str(tmp_path / "x" / "x"), mixed["names"], mixed["files"], codon_phased=True,
                                       min_count=3, **kw)
    assert mixed["calls"] == []


def test_constructDatabase_writes_one_database_with_reads_flags(mixed, tmp_path, capsys):
    db = str(tmp_path / "both" / "both")
    assert pp_sketchlib.constructDatabase(db, mixed["names"], mixed["files"], [13, 21], 64, min_count=2) == mixed["names"]
    path, _ = pp_sketchlib._db_path(db)
    assert sketchdb.reads_flags(path, mixed["names"]) == [True, False, True, False]
    assert sketchdb.reads_flags(path, ["a1", "r0"]) == [False, True]
    loaded = sketchdb.load(db, mixed["names"], [13, 21])
    assert loaded.lengths.tolist() == [1002, 10, 1008, 11]
    pp_sketchlib.addRandom(db, mixed["names"], [13, 21])          # the rewrite keeps the flags
    assert sketchdb.reads_flags(path, mixed["names"]) == [True, False, True, False]


def test_an_assembly_only_database_is_byte_for_byte_what_it_was(tmp_path):
    from poppunk_amd import synth
    sk, _ = synth.make_sketches(3, [13, 17], sketchsize64=2, cluster_size=3)
    kw = dict(lengths=[10, 20, 30], base_freq=np.full((3, 4), 0.25), missing_bases=[1, 2, 3])
    forms = [("npz", sketchdb.save_npz)]
    try:
        sketchdb._h5_backend()
        forms.append(("h5", sketchdb.save_h5))
    except ImportError:
        pass
    for ext, save in forms:
        plain, absent, flagged = (str(tmp_path / (ext + x) / "db") for x in ("0", "1", "2"))
        save(plain, ["a", "b", "c"], [13, 17], sk, 2, 14, **kw)
        save(absent, ["a", "b", "c"], [13, 17], sk, 2, 14, reads=None, **kw)
        save(flagged, ["a", "b", "c"], [13, 17], sk, 2, 14, reads=[0, 1, 0], **kw)
        assert open(plain + "." + ext, "rb").read() == open(absent + "." + ext, "rb").read()
        assert sketchdb.reads_flags(plain + "." + ext, ["a", "b", "c"]) is None
        assert sketchdb.reads_flags(flagged + "." + ext, ["c", "b"]) == [False, True]
        assert np.array_equal(sketchdb.load(flagged, ["a", "b", "c"], [13, 17]).sketches, sk)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

def _call(codes, off, kmers, s64=1, bbits=14, flags=0, min_count=2, device=0, dev_call=False):
    lib = _lib.lib()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    k = np.ascontiguousarray(kmers, dtype=np.int32)
    n = len(off) - 1
    sk = np.zeros((max(n, 1), max(len(k), 1), max(s64, 1) * 14), dtype=np.uint64)
    st = np.zeros((max(n, 1), 6), dtype=np.int64)
    kst = np.zeros((max(n, 1), max(len(k), 1), 4), dtype=np.int64)
    fl = np.zeros((max(n, 1), max(len(k), 1)), dtype=np.int32)
    if dev_call:      # (host pointers: every one of these errors is found before they would be read)
        return lib.ppk_sketch_reads_dev(codes.ctypes.data, off.ctypes.data, n, k.ctypes.data_as(C.POINTER(C.c_int32)), len(k),
                                        s64, bbits, flags, min_count, sk.ctypes.data, st.ctypes.data, kst.ctypes.data,
                                        fl.ctypes.data, None)
    return lib.ppk_sketch_reads(codes.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data_as(C.POINTER(C.c_longlong)), n,
                                k.ctypes.data_as(C.POINTER(C.c_int32)), len(k), s64, bbits, flags, min_count, device,
                                sk.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(C.POINTER(C.c_longlong)),
                                kst.ctypes.data_as(C.POINTER(C.c_longlong)), fl.ctypes.data_as(C.POINTER(C.c_int32)))


@pytest.mark.parametrize("dev_call", [False, True])
def test_argument_errors_are_returned_by_code(dev_call):
    lib = _lib.lib()
    codes, off = np.zeros(64, dtype=np.uint8), [0, 30, 64]
    assert _lib.SKETCH_EXACT == 2 and _lib.SKETCH_STRAND_PRESERVED == 1
    for kwargs, message in ((dict(kmers=[2]), b"k-mer length 2 outside 3 .. 101"),
                            (dict(kmers=[13, 102]), b"k-mer length 102 outside 3 .. 101"),
                            (dict(kmers=[]), b"nk must be 1 .. 128"),
                            (dict(kmers=[13], bbits=12), b"bbits must be 14"),
                            (dict(kmers=[13], s64=0), b"sketchsize64 must be at least 1"),
                            (dict(kmers=[13], s64=4097), b"sketchsize64 above 4096"),
                            (dict(kmers=[13], flags=4), b"unknown flag"),
                            (dict(kmers=[13], flags=8 | 2), b"unknown flag"),
                            (dict(kmers=[13], min_count=0), b"min_count 0 outside 1 .. 65535"),
                            (dict(kmers=[13], min_count=-3), b"min_count -3 outside 1 .. 65535"),
                            (dict(kmers=[13], min_count=65536), b"min_count 65536 outside 1 .. 65535")):
        assert _call(codes, off, dev_call=dev_call, **kwargs) == _lib.ERR_ARG, kwargs
        assert b"ppk_sketch_reads: " + message in lib.ppk_last_error(), (kwargs, lib.ppk_last_error())
    assert _call(codes, [0], kmers=[13], flags=3, dev_call=dev_call) == _lib.OK      # no sample: nothing to do
    if not dev_call:
        assert _call(codes, off, kmers=[13], device=64) == _lib.ERR_ARG and b"out of range [0, 64)" in lib.ppk_last_error()
        assert _call(codes, off, kmers=[], device=-1) == _lib.ERR_ARG and b"out of range [0, 64)" in lib.ppk_last_error()
        assert _call(codes, [0, 40, 30], kmers=[13]) == _lib.ERR_ARG
        assert b"ppk_sketch_reads: offsets do not ascend at sample 1" in lib.ppk_last_error()
        assert lib.ppk_sketch_reads(None, None, 1, None, 1, 1, 14, 0, 2, 0, None, None, None, None) == _lib.ERR_ARG
        assert b"NULL array" in lib.ppk_last_error()


def test_read_options_are_in_the_option_table_and_checked():
    lib = _lib.lib()
    for name, default in (("sketch_count_bits", 0), ("sketch_exact_rounds", 64)):
        if "PPK_" + name.upper() not in os.environ:
            assert _lib.get_option(name) == default
    codes, off = np.zeros(64, dtype=np.uint8), [0, 64]
    old = _lib.get_option("sketch_count_bits"), _lib.get_option("sketch_exact_rounds")
    try:
        for bits in (3, 27, -1):
            _lib.set_option("sketch_count_bits", bits)
            assert _call(codes, off, kmers=[13]) == _lib.ERR_ARG
            assert b"option sketch_count_bits must be 0 or 4 .. 26" in lib.ppk_last_error()
        _lib.set_option("sketch_count_bits", 12)
        _lib.set_option("sketch_exact_rounds", 0)
        assert _call(codes, off, kmers=[13]) == _lib.ERR_ARG and b"sketch_exact_rounds must be at least 1" in lib.ppk_last_error()
    finally:
        _lib.set_option("sketch_count_bits", old[0])
        _lib.set_option("sketch_exact_rounds", old[1])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_sketching_reads_without_a_gpu_is_an_error_not_a_fallback(tmp_path):
    assert _call(np.zeros(64, dtype=np.uint8), [0, 64], kmers=[13]) == _lib.ERR_HIP
    (tmp_path / "r.fq").write_bytes(b"@r\n" + b"ACGTTGCA" * 20 + b"\n+\n" + b"I" * 160 + b"\n")
    with pytest.raises(RuntimeError):
        sketching.sketch_files(["r"], [str(tmp_path / "r.fq")], [13], 64, min_count=1)
