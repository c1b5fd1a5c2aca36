"""GPU tests of the sketcher (ppk_sketch*, engine.sketch_dev, poppunk_amd.sketching, constructDatabase).
Words, statistics and filled counts are compared with the numpy restatement (tests/sketch_model.py) with array_equal at
every length, k-mer length and sketch size where the kernels take another path; the routes (LDS minima / global
atomics, forced batches, host / device call) against one another; the first-offender errors by message; and FASTA
files -> constructDatabase -> queryDatabase against the same query on the model's sketches, bit for bit.

The hash kernel cuts a sample into pieces of start positions (poppunk_amd/csrc/ppk_sketch.hip; test_sketch_host.py
checks that the source still says so): a lane rolls through LANE of them, a wave through WAVE, a workgroup through WG."""
import os

import numpy as np
import pytest

import sketch_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, pp_sketchlib, sketchdb, sketching, sketchlib, synth  # noqa: E402

DEV = "cuda:0"
LANE, WAVE, WG = 128, 8192, 65536          # kLanePiece, kWavePiece, kWgPiece
LDS_BINS = 20352                           # the most bins whose minima the hash kernel keeps in LDS (159 KiB)
BEYOND_LDS = 320                           # sketchsize64 of 20 480 bins: the global-atomics route


def genome(rng, length, n_other=0):
    g = sm.random_genome(rng, length)
    if n_other and length:
        g[rng.integers(0, length, size=n_other)] = 4
    return g


def pack(samples):
    off = np.zeros(len(samples) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in samples], out=off[1:])
    codes = np.concatenate(samples).astype(np.uint8) if samples else np.zeros(0, dtype=np.uint8)
    return codes, off


def on_device(codes, off, kmers, s64, strand_preserved=False):
    t = torch.as_tensor(codes if codes.size else np.zeros(1, dtype=np.uint8), device=DEV)
    sk, st, fl = engine.sketch_dev(t, off, kmers, s64, 14, strand_preserved)
    return sk.cpu().numpy().view(np.uint64), st.cpu().numpy(), fl.cpu().numpy()


def check(samples, kmers, s64, strand_preserved=False):
    codes, off = pack(samples)
    got = on_device(codes, off, kmers, s64, strand_preserved)
    want = sm.sketch(codes, off, kmers, s64, 14, strand_preserved)
    for g, w, what in zip(got, want, ("words", "stats", "filled")):
        assert np.array_equal(g, w), (what, kmers, s64, np.argwhere(g != w)[:5].tolist())
    return got


# ---- shape sweeps -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 13, 31, 32, 33, 63, 64, 65, 101])
def test_lengths_at_every_piece_edge(k):
    """Lengths 0, k - 1, k, k + 1, 63, 64, 65, and one less than, exactly and one more than each piece: counted in
    start positions (what a lane, a wave and a workgroup cut by) and in codes (what the piece table cuts by)."""
    rng = np.random.Generator(np.random.PCG64(1000 + k))
    lengths = [0, k - 1, k, k + 1, 63, 64, 65]
    for piece in (LANE, WAVE, WG):
        lengths += [piece + k - 1 + d for d in (-1, 0, 1)] + [piece + d for d in (-1, 0, 1)]
    check([genome(rng, n, n_other=min(2, n // 40)) for n in lengths], [k], 2)


@pytest.mark.parametrize("s64,options", [(1, {}), (2, {}), (16, {}), (156, {}), (BEYOND_LDS, {}),
                                         (16, {"sketch_lds_bins": 512}), (318, {})])
@pytest.mark.parametrize("kmers", [[21], [13, 15, 17, 19, 21, 23, 25, 27, 29]])
def test_sketch_sizes_and_both_routes(s64, options, kmers, ppk_option):
    """sketchsize64 1, 2, 16, 156 and 318 (the most LDS holds) keep their minima in LDS; 320 is beyond it, and option
    sketch_lds_bins sends 16 the same way.  nk 1 and 9."""
    assert (64 * s64 > LDS_BINS) == (s64 == BEYOND_LDS)
    for name, value in options.items():
        ppk_option(name, value)
    rng = np.random.Generator(np.random.PCG64(7 * s64 + len(kmers)))
    check([genome(rng, 20_011, 3), genome(rng, 150), genome(rng, WAVE + 77)], kmers, s64)


# ---- invalid positions --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", [LANE, WAVE, WG])
def test_an_invalid_code_at_each_position_round_a_piece_boundary(boundary):
    """A code 4 and a code 5 at each position from k - 1 before to k - 1 after the boundary, one sample each, at 9 984
    bins.  The samples of the lane and wave boundaries are short, so that nearly every k-mer is its bin's minimum and a
    k-mer wrongly kept or dropped shows; at the workgroup boundary (6.6 k-mers per bin) about one in seven does."""
    k = 13
    rng = np.random.Generator(np.random.PCG64(boundary))
    base = genome(rng, boundary + 3 * k)
    samples = []
    for d in range(-(k - 1), k):
        for code in (4, 5):
            g = base.copy()
            g[boundary + d] = code
            samples.append(g)
    got = check(samples, [k], 156)
    # a 4 and a 5 at one position drop the same k-mers; the positions are not all alike
    assert np.array_equal(got[0][0::2], got[0][1::2])
    assert len({w.tobytes() for w in got[0]}) > (20 if boundary < WG else 1)


def test_invalid_codes_at_the_ends_and_an_all_n_sample(tmp_path):
    rng = np.random.Generator(np.random.PCG64(3))
    g = genome(rng, 700)
    first, last, both = g.copy(), g.copy(), g.copy()
    first[0], last[-1] = 4, 5
    both[0], both[-1] = 5, 4
    all_n = np.full(300, 4, dtype=np.uint8)
    breaks = np.full(40, 5, dtype=np.uint8)
    words, stats, filled = check([first, last, both, all_n, breaks, g], [13, 21], 16)
    assert filled[3].tolist() == [0, 0] and not words[3].any() and stats[3].tolist() == [300, 300, 0, 0, 0, 0]
    assert filled[4].tolist() == [0, 0] and not words[4].any() and stats[4].tolist() == [0, 0, 0, 0, 0, 0]
    # the Python layer names the samples it cannot sketch
    codes, off = pack([g, all_n])
    with pytest.raises(RuntimeError, match=r"no valid k-mer to sketch in 1 sample\(s\): enns \(k = 13,21\)"):
        sketching.sketch_codes(codes, off, [13, 21], 1024, names=["fine", "enns"])
    (tmp_path / "fine.fa").write_text(">f\n" + "".join("ACGT"[c] for c in g) + "\n")
    (tmp_path / "enns.fa").write_text(">n\n" + "N" * 300 + "\n")
    with pytest.raises(RuntimeError, match="enns"):
        sketching.sketch_to_db(["fine", "enns"], [str(tmp_path / "fine.fa"), str(tmp_path / "enns.fa")], [13], 1024)


# ---- mixed lengths -------------------------------------------------------------------------------------------------

def test_samples_of_1_base_100_bases_and_100_kb_in_one_call():
    rng = np.random.Generator(np.random.PCG64(4))
    check([genome(rng, 1), genome(rng, 100), genome(rng, 100_000, 5), genome(rng, 100), genome(rng, 1)], [13, 21], 16)


# ---- routes and repeatability -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seven():
    rng = np.random.Generator(np.random.PCG64(8))
    samples = [genome(rng, n, n // 300) for n in (0, 50, 300, 9000, 70_000, 12, 2500)]
    codes, off = pack(samples)
    kmers = [13, 29]
    return codes, off, kmers, {sp: sm.sketch(codes, off, kmers, 16, 14, sp) for sp in (False, True)}


@pytest.mark.parametrize("strand_preserved", [False, True])
def test_host_call_device_call_and_model_agree(seven, strand_preserved):
    codes, off, kmers, want = seven
    dev = on_device(codes, off, kmers, 16, strand_preserved)
    again = on_device(codes, off, kmers, 16, strand_preserved)
    for d, a, w in zip(dev, again, want[strand_preserved]):
        assert np.array_equal(d, w) and np.array_equal(d, a)
    assert not np.array_equal(want[False][0], want[True][0])
    # the host call: sample 0 and sample 5 have no k-mer, which the Python layer refuses -- so through the ABI
    import ctypes as C
    n, nk = len(off) - 1, len(kmers)
    sk = np.zeros((n, nk, 16 * 14), dtype=np.uint64)
    st = np.zeros((n, 6), dtype=np.int64)
    fl = np.zeros((n, nk), dtype=np.int32)
    k = np.asarray(kmers, dtype=np.int32)
    rc = _lib.lib().ppk_sketch(codes.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data_as(C.POINTER(C.c_longlong)),
                               n, k.ctypes.data_as(C.POINTER(C.c_int32)), nk, 16, 14, 1 if strand_preserved else 0, 0,
                               sk.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(C.POINTER(C.c_longlong)),
                               fl.ctypes.data_as(C.POINTER(C.c_int32)))
    _lib.check(rc, "ppk_sketch")
    for h, w in zip((sk, st, fl), want[strand_preserved]):
        assert np.array_equal(h, w)


@pytest.mark.parametrize("options", [{"sketch_batch": 1}, {"sketch_batch": 2}, {"sketch_batch": 3},
                                     {"sketch_lds_bins": 64}])
def test_forced_batches_and_routes_equal_one_batch(seven, options, ppk_option):
    codes, off, kmers, want = seven
    keep = [2, 3, 4, 6, 1]                      # (the samples that have a k-mer of both lengths; 50 bases has k = 13, 29)
    samples = [codes[off[i]:off[i + 1]] for i in keep]
    c, o = pack(samples)
    for name, value in options.items():
        ppk_option(name, value)
    got = sketching.sketch_codes(c, o, kmers, 16 * 64)
    for g, w in zip(got, want[False]):
        assert np.array_equal(g, w[keep])


# ---- bad input ------------------------------------------------------------------------------------------------------

def test_bad_codes_and_offsets_are_reported_by_message():
    rng = np.random.Generator(np.random.PCG64(6))
    samples = [genome(rng, 500), genome(rng, 70_000), genome(rng, 300)]
    samples[1][66_000] = 9
    samples[1][69_000] = 200
    samples[2][5] = 6
    codes, off = pack(samples)
    with pytest.raises(RuntimeError, match=r"ppk_sketch: sample 1, position 66000 \(code 66500\): code 9 above 5"):
        on_device(codes, off, [13], 2)
    with pytest.raises(RuntimeError, match=r"ppk_sketch: sample 1, position 66000 \(code 66500\): code 9 above 5"):
        sketching.sketch_codes(codes, off, [13], 128)
    # ... also when the batch that holds it is not the first
    _lib.set_option("sketch_batch", 1)
    try:
        with pytest.raises(RuntimeError, match=r"ppk_sketch: sample 1, position 66000 \(code 66500\): code 9 above 5"):
            sketching.sketch_codes(codes, off, [13], 128)
    finally:
        _lib.set_option("sketch_batch", 0)
    samples[1][66_000], samples[1][69_000], samples[2][5] = 0, 0, 0
    codes, off = pack(samples)
    bad = off.copy()
    bad[2] = off[1] - 1
    with pytest.raises(RuntimeError, match="ppk_sketch: offsets do not ascend at sample 1"):
        on_device(codes, bad, [13], 2)
    with pytest.raises(RuntimeError, match="ppk_sketch: offsets do not ascend at sample 1"):
        sketching.sketch_codes(codes, bad, [13], 128)
    check(samples, [13], 2)                     # the next call is not disturbed


# ---- end to end ---------------------------------------------------------------------------------------------------------

def write_fasta(path, records, width=70):
    with open(path, "w") as f:
        for i, codes in enumerate(records):
            f.write(">contig_%d\n" % i)
            text = "".join("ACGTN"[c] for c in codes)
            for a in range(0, len(text), width):
                f.write(text[a:a + width] + "\n")


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    """three related genomes of 30 kb in two contigs each, as FASTA files, a listing and the model's sketches"""
    root = tmp_path_factory.mktemp("family")
    rng = np.random.Generator(np.random.PCG64(12))
    g = sm.random_genome(rng, 30_000)
    names, files, samples = [], [], []
    for i, pi in enumerate((0.0, 0.01, 0.03)):
        m = sm.mutate(rng, g, pi)
        m[1000 + i] = 4
        cut = 12_000 + 100 * i
        path = str(root / ("g%d.fa" % i))
        write_fasta(path, [m[:cut], m[cut:]])
        names.append("g%d" % i)
        files.append(path)
        samples.append(np.concatenate([m[:cut], [5], m[cut:]]).astype(np.uint8))
    listing = str(root / "rfile.txt")
    with open(listing, "w") as f:
        for nm, path in reversed(list(zip(names, files))):
            f.write(nm + "\t" + path + "\n")
    kmers = [13, 17, 21, 25, 29]
    codes, off = pack(samples)
    return dict(root=root, names=names, files=files, listing=listing, kmers=kmers,
                model=sm.sketch(codes, off, kmers, 16, 14))


def test_fasta_to_distances_equals_the_model_sketches(family):
    f = family
    prefix = str(f["root"] / "made")
    names = sketchlib.constructDatabase(f["listing"], f["kmers"], 1024, prefix, threads=2, overwrite=False,
                                        strand_preserved=False, min_count=0, use_exact=False)
    assert names == f["names"]
    got = sketchlib.queryDatabase(names, names, prefix, prefix, f["kmers"], self=True)
    words, stats, _ = f["model"]
    table = synth.random_match_table(f["kmers"], genome_length=float(stats[:, 0].mean()))
    forms = [("npz", sketchdb.save_npz)]
    try:
        sketchdb._h5_backend()
        forms.append(("h5", sketchdb.save_h5))
    except ImportError:
        pass
    for form, save in forms:
        db = str(f["root"] / form / form)
        save(db, names, f["kmers"], words, 16, 14, random_table=table, clusters=np.zeros(3, dtype=np.uint16),
             lengths=stats[:, 0])
        want = pp_sketchlib.queryDatabase(db, db, names, names, f["kmers"], random_correct=True)
        assert got.shape == (3, 2) and np.array_equal(got, want), form
    assert 0 < got[0, 0] < got[1, 0] and got[2, 0] > 0          # (g1, g0) closer than (g2, g0)
    # addRandom's table is the documented J_r(k) at the mean sketched length, one cluster
    loaded = sketchdb.load(prefix + "/made", names, f["kmers"])
    assert np.array_equal(loaded.random_table, table) and loaded.random_status == "mapped"
    assert np.array_equal(loaded.sketches, words)
    assert loaded.lengths.tolist() == stats[:, 0].tolist() and loaded.missing_bases.tolist() == [1, 1, 1]
    uncorrected = pp_sketchlib.queryDatabase(prefix + "/made", prefix + "/made", names, names, f["kmers"], random_correct=False)
    assert uncorrected.shape == got.shape


def test_sketch_to_db_gives_the_same_rows_without_a_file(family):
    f = family
    db, stats, filled = sketching.sketch_to_db(f["names"], f["files"], f["kmers"], 1024)
    words, want_stats, want_filled = f["model"]
    assert np.array_equal(stats, want_stats) and np.array_equal(filled, want_filled)
    table = synth.random_match_table(f["kmers"], genome_length=float(want_stats[:, 0].mean()))
    ref = engine.SketchDB(words, 16, 14, device=0)
    got, _ = engine.dist(db, None, f["kmers"], table)
    want, _ = engine.dist(ref, None, f["kmers"], table)
    assert torch.equal(got, want)
    db.close()
    ref.close()
