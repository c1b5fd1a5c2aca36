"""CPU tests of the sketcher, no GPU: the numpy restatement of the rule (tests/sketch_model.py) against
hand values and as an estimator of the Jaccard index, the ppk_device.h helpers run on the host against the model
(sketch_device_host.hip), read_fasta, readRfile, sketchlibAssemblyQC against the reference's answers
(tests/golden/sketch_qc.json) and the argument errors of the C ABI.

[EXT] The rule is this project's own: what stands in for parity with pp-sketchlib is the estimator test."""
import ctypes as C
import gzip
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sketch_model as sm
from poppunk_amd import _lib, qc, sketchdb, sketching, utils

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M64 = (1 << 64) - 1
A, Cc, G, T = 0x3c8bfbb395c60474, 0x3193c18562a02b4c, 0x20323ed082572324, 0x295549f54be24456


def irol(x, r):
    r %= 64
    return ((x << r) | (x >> (64 - r))) & M64 if r else x


# ---- the model against hand values ------------------------------------------------------------------------------

def test_acg_at_k3_by_hand():
    f = irol(A, 2) ^ irol(Cc, 1) ^ G                     # forward: seed[s_i] rotated by k - 1 - i
    r = T ^ irol(G, 1) ^ irol(Cc, 2)                     # reverse: the complements, rotated by i
    pos, h = sm.hashes([0, 1, 2], 3)
    assert pos.tolist() == [0] and int(h[0]) == min(f, r)
    assert int(sm.hashes([0, 1, 2], 3, strand_preserved=True)[1][0]) == f
    # the reverse complement CGT has the two hashes swapped
    pos, h = sm.hashes([1, 2, 3], 3, strand_preserved=True)
    assert int(h[0]) == r


def test_rotation_amounts_are_taken_mod_64():
    for k in (64, 65, 101):
        codes = (np.arange(k) * 7 % 4).astype(np.uint8)
        f = 0
        for i, s in enumerate(codes.tolist()):
            f ^= irol((A, Cc, G, T)[s], (k - 1 - i) % 64)
        assert int(sm.hashes(codes, k, strand_preserved=True)[1][0]) == f


def test_reverse_complement_gives_the_same_sketch_and_strand_preserved_differs():
    rng = np.random.Generator(np.random.PCG64(5))
    g = sm.random_genome(rng, 5000)
    g[100], g[3000] = 4, 5
    rc = sm.reverse_complement(g)
    off = [0, len(g)]
    for k in (13, 32, 33):
        w0, s0, f0 = sm.sketch(g, off, [k], 2)
        w1, s1, f1 = sm.sketch(rc, off, [k], 2)
        assert np.array_equal(w0, w1) and np.array_equal(f0, f1)
        assert s0[0, 0] == s1[0, 0] and s0[0, 1] == s1[0, 1] and s0[0, 2:].tolist() == s1[0, 2:][::-1].tolist()
        p0 = sm.sketch(g, off, [k], 2, strand_preserved=True)[0]
        p1 = sm.sketch(rc, off, [k], 2, strand_preserved=True)[0]
        assert not np.array_equal(p0, p1) and not np.array_equal(p0, w0)


def test_windows_never_span_a_code_of_4_or_5():
    codes = np.array([0, 1, 2, 3, 4, 0, 1, 2, 5, 3, 2, 1, 0], dtype=np.uint8)
    assert sm.hashes(codes, 3)[0].tolist() == [0, 1, 5, 9, 10]
    assert sm.hashes(codes, 4)[0].tolist() == [0, 9]
    assert sm.hashes(codes, 5)[0].tolist() == []
    assert sm.stats(codes).tolist() == [12, 1, 3, 3, 3, 2]


def test_every_hash_lands_in_a_bin_below_nbins():
    edge = np.array([0, 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64], dtype=np.uint64)
    for nbins in (64, 128, 1024, 9984, 20480, 262144):
        b = sm.bin_of(edge, nbins)
        assert b.tolist() == [(int(h) * nbins) >> 64 for h in edge.tolist()]
        assert b.min() == 0 and b.max() == nbins - 1
    assert sm.keep(edge).tolist() == [0, 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64 - 1]


def test_densify():
    nbins = 128
    m = np.full(nbins, sm.EMPTY, dtype=np.uint64)
    v, filled = sm.densify(m)
    assert filled == 0 and not v.any()                    # nothing to take a value from: all zero
    m[70] = np.uint64(0x12345)                            # one filled bin: every bin takes its low 14 bits
    v, filled = sm.densify(m)
    assert filled == 1 and (v == 0x2345).all()
    m = np.full(nbins, sm.EMPTY, dtype=np.uint64)
    m[nbins - 1] = np.uint64(7)                           # only the last bin: the wrap
    v, filled = sm.densify(m)
    assert filled == 1 and (v == 7).all()
    m = (np.arange(nbins, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    v, filled = sm.densify(m)                             # all filled: nothing moves
    assert filled == nbins and np.array_equal(v, (m & np.uint64(0x3fff)).astype(np.int64))
    m[[0, 1, 64, 127]] = sm.EMPTY                         # the nearest non-empty bin ABOVE, cyclically
    v, _ = sm.densify(m)
    assert v[0] == v[2] and v[1] == v[2] and v[64] == v[65] and v[127] == v[2]


def test_bitslice_is_the_layout_of_synth():
    from poppunk_amd import synth
    rng = np.random.Generator(np.random.PCG64(9))
    vals = rng.integers(0, 1 << 14, size=256)
    assert np.array_equal(sm.bitslice(vals), synth.bitslice(vals, 14))


# ---- the sketch as an estimator: what stands in for upstream parity -------------------------------------------------

ESTIMATOR_SEED = 20261020      # observed z-scores of the model at this seed: DESIGN.md 3.23 (the largest is 1.66)


@pytest.fixture(scope="module")
def genome_family():
    rng = np.random.Generator(np.random.PCG64(ESTIMATOR_SEED))
    g = sm.random_genome(rng, 100_000)
    return g, {pi: sm.mutate(rng, g, pi) for pi in (0.001, 0.01, 0.05)}


@pytest.mark.parametrize("pi", [0.001, 0.01, 0.05])
@pytest.mark.parametrize("k", [13, 21, 29])
def test_equal_bins_estimate_the_jaccard_index(genome_family, pi, k):
    """The fraction of equal bins of two sketches (sketchsize64 = 16) lies within 4 binomial standard errors
    sqrt(J (1 - J) / nbins) of the exact Jaccard index J of the two genomes' k-mer hash sets."""
    g, mutants = genome_family
    nbins = 16 * 64
    va, _ = sm.densify(sm.minima(g, k, nbins))
    vb, _ = sm.densify(sm.minima(mutants[pi], k, nbins))
    jac = sm.jaccard(g, mutants[pi], k)
    se = (jac * (1.0 - jac) / nbins) ** 0.5
    z = (sm.equal_bins(va, vb) - jac) / se
    print("pi %g k %d: J %.4f, equal bins %.4f, z %+.2f" % (pi, k, jac, sm.equal_bins(va, vb), z))
    assert abs(z) <= 4.0


# ---- the device helpers on the host ----------------------------------------------------------------------------------

def test_kernel_piece_constants_are_the_ones_the_gpu_tests_name():
    src = open(os.path.join(ROOT, "poppunk_amd", "csrc", "ppk_sketch.hip")).read()
    assert int(re.search(r"kLanePiece = (\d+);", src).group(1)) == 128
    assert int(re.search(r"kThreads = (\d+);", src).group(1)) == 512
    assert "kWavePiece = 64 * kLanePiece;" in src and "kWgPiece = (kThreads / 64) * kWavePiece;" in src


def test_sketch_helpers_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    rng = np.random.Generator(np.random.PCG64(11))
    lines = []
    for k, sp, nbins, length in ((3, 0, 64, 40), (13, 0, 1024, 400), (31, 1, 9984, 300), (32, 0, 128, 300),
                                 (33, 0, 20480, 300), (63, 1, 64, 200), (64, 0, 1024, 200), (65, 0, 1024, 200),
                                 (101, 0, 9984, 350)):
        codes = sm.random_genome(rng, length)
        codes[rng.integers(0, length, size=3)] = [4, 5, 4]
        lines.append("S %d %d %d %s" % (k, sp, nbins, "".join(map(str, codes.tolist()))))
        pos, h = sm.hashes(codes, k, bool(sp))
        for p, hv, b in zip(pos.tolist(), h.tolist(), sm.bin_of(h, nbins).tolist()):
            lines.append("V %d %x %d" % (p, hv, b))
        lines.append("E")
    for nbins in (64, 1024, 9984, 262144):
        for hv in (0, 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64):
            lines.append("B %x %d %d" % (hv, nbins, (hv * nbins) >> 64))
    lines += ["K %x %x" % (M64, M64 - 1), "K %x %x" % (M64 - 1, M64 - 1), "K 0 0"]
    nbins = 320
    for full in ([5], [nbins - 1], [0], list(range(nbins)), [3, 64, 65, 200], [130, 131], [63, 64], [319, 0]):
        m = np.full(nbins, sm.EMPTY, dtype=np.uint64)
        m[full] = np.arange(len(full), dtype=np.uint64)
        ne = np.flatnonzero(m != sm.EMPTY)
        src = ne[np.searchsorted(ne, np.arange(nbins)) % ne.size]
        lines.append("M %d %s" % (nbins, " ".join(map(str, sorted(full)))))
        lines.append("R " + " ".join(map(str, src.tolist())))
    records = tmp_path / "records.txt"
    records.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "sketch_device_host")
    # The sanitizers are for the host code alone: -Xarch_host keeps them off any device pass.
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17",
                          "-Xarch_host", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                          os.path.join(HERE, "sketch_device_host.hip"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe, str(records)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert " 0 wrong" in run.stdout
    assert int(run.stdout.split()[0]) > 5000


# ---- read_fasta ---------------------------------------------------------------------------------------------------

def test_read_fasta_forms(tmp_path):
    want = [0, 1, 2, 3, 4, 4, 0, 0, 5, 3, 3, 2, 4, 1]
    text = ">one some words > more\nACGTNRaa\n>two\nTTG\nYc\n"
    forms = {"plain.fa": text.encode(), "crlf.fa": text.replace("\n", "\r\n").encode(),
             "no_final_newline.fa": text[:-1].encode(), "lower.fa": text.lower().replace(">one", ">one").encode(),
             "blank_lines.fa": ("\n\n" + text.replace("TTG\n", "TTG\n\n")).encode()}
    for name, data in forms.items():
        (tmp_path / name).write_bytes(data)
        assert sketching.read_fasta(str(tmp_path / name)).tolist() == want, name
    with gzip.open(tmp_path / "packed.fa.gz", "wb") as f:
        f.write(text.encode())
    got = sketching.read_fasta(str(tmp_path / "packed.fa.gz"))
    assert got.dtype == np.uint8 and got.tolist() == want
    (tmp_path / "single.fa").write_bytes(b">x\nACGT")
    assert sketching.read_fasta(str(tmp_path / "single.fa")).tolist() == [0, 1, 2, 3]
    (tmp_path / "header_only.fa").write_bytes(b">x")
    assert sketching.read_fasta(str(tmp_path / "header_only.fa")).tolist() == []
    # every IUPAC letter, '-' and '*' are "any other residue"
    (tmp_path / "iupac.fa").write_bytes(b">x\nRYSWKMBDHVNU-*\n")
    assert set(sketching.read_fasta(str(tmp_path / "iupac.fa")).tolist()) == {4}


def test_read_fasta_errors(tmp_path):
    (tmp_path / "empty.fa").write_bytes(b"")
    (tmp_path / "blank.fa").write_bytes(b"\n\n")
    for name in ("empty.fa", "blank.fa"):
        with pytest.raises(ValueError, match="is empty"):
            sketching.read_fasta(str(tmp_path / name))
    (tmp_path / "reads.fq").write_bytes(b"@r1\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError, match="FASTQ"):
        sketching.read_fasta(str(tmp_path / "reads.fq"))
    (tmp_path / "text.fa").write_bytes(b"ACGT\n")
    with pytest.raises(ValueError, match="not FASTA"):
        sketching.read_fasta(str(tmp_path / "text.fa"))
    with pytest.raises(OSError):
        sketching.read_fasta(str(tmp_path / "missing.fa"))


def test_read_samples_joins_files_and_counts_offsets(tmp_path):
    (tmp_path / "a.fa").write_bytes(b">a\nAC\n")
    (tmp_path / "b.fa").write_bytes(b">b\nGT\n>c\nN\n")
    a, b = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
    for threads in (1, 4, 64):
        codes, off = sketching.read_samples([a, [a, b], [b]], threads)
        assert off.tolist() == [0, 2, 9, 13]
        assert codes.tolist() == [0, 1, 0, 1, 5, 2, 3, 5, 4, 2, 3, 5, 4]
    assert sketching.MAX_READ_THREADS == 16
    with pytest.raises(ValueError, match="at least 64"):
        sketching.sketchsize64_of(63)
    assert sketching.sketchsize64_of(10000) == 156
    assert np.allclose(sketching.base_freq_of([[10, 0, 1, 2, 3, 4], [0, 0, 0, 0, 0, 0]]),
                       [[0.1, 0.2, 0.3, 0.4], [0.25] * 4])
    with pytest.raises(RuntimeError, match=r"no valid k-mer.*b \(k = 21\)"):
        sketching.check_filled(np.array([[3, 4], [5, 0]]), ["a", "b"], [13, 21])


# ---- readRfile ------------------------------------------------------------------------------------------------------

def test_readRfile(tmp_path, capsys):
    listing = tmp_path / "rfile.txt"
    listing.write_text("zeta.1\t/data/z.fa\nalpha(2)\t/data/a_1.fa\t/data/a_2.fa\nmid:x\t/data/m.fa\n")
    names, seqs = utils.readRfile(str(listing))
    assert names == ["alpha_2_", "midx", "zeta_1"]
    assert seqs == [["/data/a_1.fa", "/data/a_2.fa"], ["/data/m.fa"], ["/data/z.fa"]]
    names, seqs = utils.readRfile(str(listing), oneSeq=True)
    assert seqs == ["/data/a_1.fa", "/data/m.fa", "/data/z.fa"]
    assert "Multiple sequence found for alpha(2). Only using first\n" in capsys.readouterr().err
    for text, message in (("only_a_name\n", "Input reference list is misformatted\n"
                                            "Must contain sample name and file, tab separated\n"),
                          ("dir/name\tf.fa\n", "Sample names may not contain slashes\n"),
                          ("a.b\tf.fa\na_b\tg.fa\n", "Input contains duplicate names! All names must be unique\n"
                                                     "Non-unique names are a_b\n")):
        listing.write_text(text)
        with pytest.raises(SystemExit) as e:
            utils.readRfile(str(listing))
        assert e.value.code == 1
        assert capsys.readouterr().err == message


# ---- sketchlibAssemblyQC --------------------------------------------------------------------------------------------

def _write_qc_db(prefix, samples):
    """`<prefix>/<basename>.h5` with the attributes the QC reads, through whichever HDF5 backend there is"""
    _, h5open = sketchdb._h5_backend()
    os.makedirs(prefix)
    f = h5open(os.path.join(prefix, os.path.basename(prefix) + ".h5"), "w")
    try:
        top = f.create_group("sketches")
        for name, (length, missing, reads) in samples.items():
            g = top.create_group(name)
            g.attrs["length"] = np.int64(length)
            g.attrs["missing_bases"] = np.int64(missing)
            if reads is not None:
                g.attrs["reads"] = bool(reads)
    finally:
        f.close()


def test_sketchlibAssemblyQC_against_the_reference(tmp_path, capsys):
    cases = json.load(open(os.path.join(HERE, "golden", "sketch_qc.json")))["cases"]
    assert len(cases) >= 6
    try:
        sketchdb._h5_backend()
        have_h5 = True
    except ImportError:
        have_h5 = False
    seen = set()
    for i, case in enumerate(cases):
        in_db = [n for n in sorted(case["samples"]) if n in case["names"]]
        lengths = {n: case["samples"][n][0] for n in in_db}
        ambiguous = {n: 0 if case["samples"][n][2] else case["samples"][n][1] for n in in_db}
        retained, failed = qc.assembly_qc_verdict(case["names"], lengths, ambiguous, case["qc_dict"])
        assert retained == case["retained"] and failed == case["failed"], case["what"]
        if have_h5:
            prefix = str(tmp_path / ("db%d" % i))
            _write_qc_db(prefix, case["samples"])
            capsys.readouterr()
            retained, failed = qc.sketchlibAssemblyQC(prefix, case["names"], case["qc_dict"])
            assert retained == case["retained"] and failed == case["failed"], case["what"]
            err = capsys.readouterr().err
            assert err.startswith("Running QC on sketches\nUsing ")
            assert ("Using count cutoff for ambiguous bases: " in err) == (case["qc_dict"]["upper_n"] is not None)
            assert ("Using range for length cutoffs: " in err) == (case["qc_dict"]["length_range"][0] is not None)
        for reasons in case["failed"].values():
            seen.add(tuple(reasons))
    assert {("Below lower length threshold",), ("Above upper length threshold",), ("Ambiguous sequence too high",),
            ("Below lower length threshold", "Ambiguous sequence too high")} <= seen


def test_missing_bases_round_trip(tmp_path):
    from poppunk_amd import synth
    sk, _ = synth.make_sketches(4, [13, 17], sketchsize64=2, cluster_size=2)
    names = ["a", "b", "c", "d"]
    kw = dict(lengths=[10, 20, 30, 40], base_freq=np.full((4, 4), 0.25))
    db = str(tmp_path / "npz" / "npz")
    sketchdb.save_npz(db, names, [13, 17], sk, 2, 14, missing_bases=[1, 2, 3, 4], **kw)
    assert sketchdb.load(db, ["c", "a"], [13, 17]).missing_bases.tolist() == [3, 1]
    db0 = str(tmp_path / "npz0" / "npz0")
    sketchdb.save_npz(db0, names, [13, 17], sk, 2, 14, **kw)         # the default output stays as it was
    assert "missing_bases" not in np.load(db0 + ".npz").files and sketchdb.load(db0, names, [13]).missing_bases is None
    try:
        sketchdb._h5_backend()
    except ImportError:
        return
    db = str(tmp_path / "h5" / "h5")
    sketchdb.save_h5(db, names, [13, 17], sk, 2, 14, missing_bases=[1, 2, 3, 4], sketch_version="poppunk_amd:sketch1", **kw)
    assert sketchdb.load(db, ["d", "b"], [17]).missing_bases.tolist() == [4, 2]
    assert [int(x) for x in sketchdb.get_database_statistics(str(tmp_path / "h5"))[1]] == [1, 2, 3, 4]


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def _call(codes, off, kmers, s64=1, bbits=14, flags=0, device=0):
    lib = _lib.lib()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    k = np.ascontiguousarray(kmers, dtype=np.int32)
    n = len(off) - 1
    sk = np.zeros((max(n, 1), max(len(k), 1), max(s64, 1) * 14), dtype=np.uint64)
    st = np.zeros((max(n, 1), 6), dtype=np.int64)
    fl = np.zeros((max(n, 1), max(len(k), 1)), dtype=np.int32)
    return lib.ppk_sketch(codes.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data_as(C.POINTER(C.c_longlong)), n,
                          k.ctypes.data_as(C.POINTER(C.c_int32)), len(k), s64, bbits, flags, device,
                          sk.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(C.POINTER(C.c_longlong)),
                          fl.ctypes.data_as(C.POINTER(C.c_int32)))


def test_argument_errors_are_returned_by_code():
    lib = _lib.lib()
    codes, off = np.zeros(64, dtype=np.uint8), [0, 30, 64]
    for kwargs, message in ((dict(kmers=[2]), b"k-mer length 2 outside 3 .. 101"),
                            (dict(kmers=[13, 102]), b"k-mer length 102 outside 3 .. 101"),
                            (dict(kmers=[]), b"nk must be 1 .. 128"),
                            (dict(kmers=[13], bbits=12), b"bbits must be 14"),
                            (dict(kmers=[13], s64=0), b"sketchsize64 must be at least 1"),
                            (dict(kmers=[13], flags=2), b"unknown flag"),
                            (dict(kmers=[13], device=64), b"out of range [0, 64)")):
        assert _call(codes, off, **kwargs) == _lib.ERR_ARG, kwargs
        assert message in lib.ppk_last_error(), (kwargs, lib.ppk_last_error())
    assert _call(codes, [0, 40, 30], kmers=[13]) == _lib.ERR_ARG
    assert b"offsets do not ascend at sample 1" in lib.ppk_last_error()
    assert _call(codes, [-1, 40], kmers=[13]) == _lib.ERR_ARG
    assert b"offsets do not ascend at sample 0" in lib.ppk_last_error()
    assert lib.ppk_sketch(None, None, 1, None, 1, 1, 14, 0, 0, None, None, None) == _lib.ERR_ARG
    assert b"NULL array" in lib.ppk_last_error()
    assert _call(codes, [0], kmers=[13]) == _lib.OK                  # no sample: nothing to do, no device needed


def test_sketch_options_are_in_the_option_table():
    for name, default in (("sketch_lds_bins", 0), ("sketch_batch_mb", 1024), ("sketch_batch", 0)):
        if "PPK_" + name.upper() not in os.environ:
            assert _lib.get_option(name) == default
        old = _lib.get_option(name)
        try:
            _lib.set_option(name, 7)
            assert _lib.get_option(name) == 7
        finally:
            _lib.set_option(name, old)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_sketching_without_a_gpu_is_an_error_not_a_fallback(tmp_path):
    assert _call(np.zeros(64, dtype=np.uint8), [0, 64], kmers=[13]) == _lib.ERR_HIP
    (tmp_path / "a.fa").write_bytes(b">a\n" + b"ACGTTGCA" * 20 + b"\n")
    with pytest.raises(RuntimeError):
        sketching.sketch_files(["a"], [str(tmp_path / "a.fa")], [13], 64)
