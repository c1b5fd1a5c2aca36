"""GPU tests of sketching read sets (ppk_sketch_reads*, engine.sketch_reads_dev, sketching.sketch_read_codes,
constructDatabase on FASTQ).  Every test compares words, filled, stats and kstats of the device with
the numpy restatement of the rule (tests/sketch_reads_model.py), bit for bit: both routes, both strand settings,
min_count 1 .. 4, the default and two forced table sizes (B = 12 makes nearly every error k-mer pass the table, so the
exact route needs its rounds), the LDS and the global route, cuts and batches, the groups the scratch caps make, one
counter asked 2.4 to 2.8 * 10^5 times, the rounds cap, and FASTQ -> constructDatabase -> queryDatabase."""
import gzip
import os

import numpy as np
import pytest

import sketch_model as sm
import sketch_reads_model as rm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, pp_sketchlib, sketchdb, sketching, synth  # noqa: E402

DEV = "cuda:0"
KMERS = [13, 21, 29]
WHAT = ("words", "stats", "kstats", "filled")


def pack(samples):
    off = np.zeros(len(samples) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in samples], out=off[1:])
    codes = np.concatenate(samples).astype(np.uint8) if samples else np.zeros(0, dtype=np.uint8)
    return codes, off


def on_device(codes, off, kmers, s64, min_count, exact=False, strand_preserved=False):
    t = torch.as_tensor(codes if codes.size else np.zeros(1, dtype=np.uint8), device=DEV)
    sk, st, fl, kst = engine.sketch_reads_dev(t, off, kmers, s64, min_count, exact, 14, strand_preserved)
    return sk.cpu().numpy().view(np.uint64), st.cpu().numpy(), kst.cpu().numpy(), fl.cpu().numpy()


def same(got, want, note):
    for g, w, what in zip(got, want, WHAT):
        assert np.array_equal(g, w), (what, note, np.argwhere(g != w)[:5].tolist())


class Samples:
    """samples with the model's kept hashes computed once per (sample, k, strand)"""

    def __init__(self, samples):
        self.samples = samples
        self.codes, self.off = pack(samples)
        self._h = {}

    def hashes(self, kmers, sp):
        for i, c in enumerate(self.samples):
            for k in kmers:
                if (i, k, sp) not in self._h:
                    self._h[(i, k, sp)] = rm.kept_hashes(c, k, sp)
        return {(i, k): self._h[(i, k, sp)] for i in range(len(self.samples)) for k in kmers}

    def model(self, kmers, s64, min_count, exact, bits, sp):
        return rm.sketch_reads(self.codes, self.off, kmers, s64, min_count, exact, bits, 14, sp, hashes=self.hashes(kmers, sp))

    def check(self, kmers, s64, min_count, exact, bits, sp):
        got = on_device(self.codes, self.off, kmers, s64, min_count, exact, sp)
        same(got, self.model(kmers, s64, min_count, exact, bits, sp), (kmers, s64, min_count, exact, bits, sp))
        return got


def forty_reads(rng):
    g = sm.random_genome(rng, 200_000)                  # (so long that few of the reads overlap)
    return rm.simulate_reads(rng, g, 40 * 100 / 200_000.0)[0]


@pytest.fixture(scope="module")
def three():
    """sample 0: the 20 000-base genome at 30x in 100-base reads with 1 % errors (about 606 000 codes: piece and lane
    boundaries fall inside reads and on breaks); sample 1: 40 reads, most bins empty and nothing admitted at
    min_count 3; sample 2: one read shorter than every k; sample 3: empty"""
    rng = np.random.Generator(np.random.PCG64(1))
    big = rm.simulate_reads(rng, sm.random_genome(rng, 20_000), 30)[0]
    small = forty_reads(rng)
    assert 600_000 < len(big) < 610_000 and len(small) == 40 * 101 - 1
    return Samples([big, small, sm.random_genome(rng, 11), np.zeros(0, dtype=np.uint8)])


@pytest.mark.parametrize("bits", [0, 16, 12])
@pytest.mark.parametrize("strand_preserved", [False, True])
def test_samples_routes_and_table_sizes_against_the_model(three, strand_preserved, bits, ppk_option):
    ppk_option("sketch_count_bits", bits)
    seen_empty = False
    for s64 in (1, 4):
        for min_count in (1, 2, 3):
            for exact in (False, True):
                _, stats, kstats, filled = three.check(KMERS, s64, min_count, exact, bits, strand_preserved)
                if min_count == 3 and (filled[1] == 0).any():
                    j = int(np.flatnonzero(filled[1] == 0)[0])
                    assert kstats[1, j, 2] == 0 and kstats[1, j, 3] == 0
                    seen_empty = True
                assert (filled[2:] == 0).all() and (stats[2:, 0] == 0).all() and (kstats[2:] == 0).all()
    assert seen_empty, "no (sample, k) of the 40-read sample was left without an admitted k-mer"


def test_the_global_minima_route(three, ppk_option):
    ppk_option("sketch_lds_bins", 32)                   # 64 bins and more go straight to global memory
    ppk_option("sketch_count_bits", 16)
    for exact in (False, True):
        three.check(KMERS, 1, 3, exact, 16, False)
        three.check(KMERS, 4, 2, exact, 16, True)


def test_min_count_1_is_the_assembly_sketch(three):
    t = torch.as_tensor(three.codes, device=DEV)
    for s64, sp in ((1, False), (4, True), (16, False)):
        words, _, kstats, filled = on_device(three.codes, three.off, KMERS, s64, 1, False, sp)
        sk, _, fl = engine.sketch_dev(t, three.off, KMERS, s64, 14, sp)
        assert np.array_equal(words, sk.cpu().numpy().view(np.uint64)) and np.array_equal(filled, fl.cpu().numpy())
        assert np.array_equal(kstats[:, :, 0], kstats[:, :, 1]) and np.array_equal(kstats[:, :, 2], filled)


def test_counts_at_the_edge(ppk_option):
    """64 random 40-mers, the i-th as i % 5 + 1 separate reads: admitted are exactly those repeated at least min_count
    times (22 table bits: no two of the 1 280 k-mers meet in a counter)."""
    rng = np.random.Generator(np.random.PCG64(4))
    k, bits = 21, 22
    mers = [sm.random_genome(rng, 40) for _ in range(64)]
    reads = [(i, mers[i]) for i in range(64) for _ in range(i % 5 + 1)]
    order = rng.permutation(len(reads))
    parts = []
    for o in order:
        parts += [reads[o][1], np.array([5], dtype=np.uint8)]
    s = Samples([np.concatenate(parts[:-1])])
    ppk_option("sketch_count_bits", bits)
    h_of = [rm.kept_hashes(m, k) for m in mers]
    assert len(np.unique(np.concatenate(h_of))) == 64 * 20
    for min_count in (2, 3, 4):
        for exact in (False, True):
            words, stats, kstats, filled = s.check([k], 4, min_count, exact, bits, False)
            keep = [i for i in range(64) if i % 5 + 1 >= min_count]
            assert kstats[0, 0, 0] == sum((i % 5 + 1) * 20 for i in range(64))
            assert kstats[0, 0, 1] == sum((i % 5 + 1) * 20 for i in keep)
            m = np.full(256, sm.EMPTY, dtype=np.uint64)
            count_of = {}
            for i in keep:
                np.minimum.at(m, sm.bin_of(h_of[i], 256), h_of[i])
                count_of.update({int(x): i % 5 + 1 for x in h_of[i]})
            values, n_filled = sm.densify(m)
            assert np.array_equal(words[0, 0], sm.bitslice(values)) and filled[0, 0] == n_filled
            assert kstats[0, 0, 3] == sum(count_of[int(x)] for x in m[m != sm.EMPTY])


@pytest.mark.parametrize("bits", [0, 12])
def test_one_hot_kmer_leaves_its_neighbours_alone(bits, ppk_option):
    """2 000 reads of 150 A's beside the 40 reads: one counter per row is asked 2.4 to 2.8 * 10^5 times"""
    rng = np.random.Generator(np.random.PCG64(5))
    hot = np.zeros((2000, 151), dtype=np.uint8)
    hot[:, 150] = 5
    s = Samples([np.concatenate([hot.reshape(-1), forty_reads(rng)])])
    ppk_option("sketch_count_bits", bits)
    for min_count, exact in ((2, False), (3, True)):
        _, _, kstats, _ = s.check(KMERS, 4, min_count, exact, bits, False)
        for j, k in enumerate(KMERS):
            assert kstats[0, j, 1] >= 2000 * (151 - k)


def test_cuts_batches_and_offsets_give_the_same_bits(three, ppk_option):
    ppk_option("sketch_count_bits", 16)
    want = three.model(KMERS, 4, 3, True, 16, False)
    for batch in (0, 1, 2):
        ppk_option("sketch_batch", batch)
        same(_host_call(three, 3, True), want, ("batch", batch))
    ppk_option("sketch_batch", 0)
    small = Samples(three.samples[1:])
    want = small.model(KMERS, 4, 2, False, 16, False)
    for shift in range(8):
        codes = np.concatenate([np.full(shift, 5, dtype=np.uint8), small.codes])
        same(on_device(codes, small.off + shift, KMERS, 4, 2), want, ("shift", shift))


def test_groups_of_samples_and_of_k(ppk_option):
    """The scratch caps cut a call into groups.  29 samples x 3 k at 262 144 bins (24 bytes a bin: 85 (sample, k) fit
    512 MiB) go as 28 samples and 1; at 26 table bits one (sample, k) fills the table scratch, so a sample goes one k
    at a time."""
    rng = np.random.Generator(np.random.PCG64(6))
    many = Samples([rm.simulate_reads(rng, sm.random_genome(rng, 300), 6, read_len=50)[0] for _ in range(29)])
    many.check(KMERS, 4096, 2, True, 0, False)
    ppk_option("sketch_count_bits", 26)
    one = Samples([rm.simulate_reads(rng, sm.random_genome(rng, 500), 8, read_len=60)[0], many.samples[0]])
    one.check(KMERS, 4, 2, False, 26, False)


def _host_call(s, min_count, exact):
    """ppk_sketch_reads through ctypes, without sketch_read_codes' refusal of a sample that has no k-mer"""
    import ctypes as C
    k = np.asarray(KMERS, dtype=np.int32)
    n = len(s.off) - 1
    sk = np.zeros((n, len(k), 4 * 14), dtype=np.uint64)
    st = np.zeros((n, 6), dtype=np.int64)
    kst = np.zeros((n, len(k), 4), dtype=np.int64)
    fl = np.zeros((n, len(k)), dtype=np.int32)
    rc = _lib.lib().ppk_sketch_reads(s.codes.ctypes.data_as(C.POINTER(C.c_uint8)), s.off.ctypes.data_as(C.POINTER(C.c_longlong)),
                                     n, k.ctypes.data_as(C.POINTER(C.c_int32)), len(k), 4, 14,
                                     _lib.SKETCH_EXACT if exact else 0, min_count, 0,
                                     sk.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(C.POINTER(C.c_longlong)),
                                     kst.ctypes.data_as(C.POINTER(C.c_longlong)), fl.ctypes.data_as(C.POINTER(C.c_int32)))
    _lib.check(rc, "ppk_sketch_reads")
    return sk, st, kst, fl


def test_the_rounds_cap_is_an_error_naming_sample_and_k(three, ppk_option):
    ppk_option("sketch_count_bits", 12)
    ppk_option("sketch_exact_rounds", 4)
    with pytest.raises(RuntimeError, match=r"sample 0, k (13|21|29): .* after 4 exact rounds") as e:
        on_device(three.codes, three.off, KMERS, 4, 3, exact=True)
    assert "\n" not in str(e.value)
    ppk_option("sketch_exact_rounds", 64)
    three.check(KMERS, 4, 3, True, 12, False)


# ---- end to end ---------------------------------------------------------------------------------------------------------

def write_fasta(path, codes):
    with open(path, "w") as f:
        f.write(">contig\n" + "".join("ACGTN"[c] for c in codes) + "\n")


def write_fastq_gz(path, codes):
    with gzip.open(path, "wb") as f:
        for i, read in enumerate(bytes(codes).split(b"\x05")):
            text = bytes(b"ACGTN"[c] for c in read)
            f.write(b"@read_%d\n" % i + text + b"\n+\n" + b"@" * len(text) + b"\n")


def test_fastq_to_distances_equals_the_model_sketches(tmp_path):
    """a gzip FASTQ read set, its own assembly and the assembly mutated at pi = 0.02, in one database"""
    rng = np.random.Generator(np.random.PCG64(2))
    g = sm.random_genome(rng, 20_000)
    reads = rm.simulate_reads(rng, g, 30)[0]
    own = rm.closed_assembly(g, 29)
    far = sm.mutate(rng, own, 0.02)
    write_fastq_gz(str(tmp_path / "reads.fq.gz"), reads)
    write_fasta(str(tmp_path / "own.fa"), own)
    write_fasta(str(tmp_path / "far.fa"), far)
    names = ["reads", "own", "far"]
    files = [str(tmp_path / "reads.fq.gz"), str(tmp_path / "own.fa"), str(tmp_path / "far.fa")]
    db = str(tmp_path / "made" / "made")
    assert pp_sketchlib.constructDatabase(db, names, files, KMERS, 1024, min_count=3, num_threads=2) == names
    path, _ = pp_sketchlib._db_path(db)
    assert sketchdb.reads_flags(path, names) == [True, False, False]
    loaded = sketchdb.load(db, names, KMERS)
    rw, rs, _, _ = rm.sketch_reads(reads, [0, len(reads)], KMERS, 16, 3)
    aw, as_, _ = sm.sketch(*pack([own, far]), KMERS, 16)
    words, lengths = np.concatenate([rw, aw]), np.concatenate([rs[:, 0], as_[:, 0]])
    assert np.array_equal(loaded.sketches, words) and loaded.lengths.tolist() == lengths.tolist()
    assert abs(int(lengths[0]) - 20_000) < 1_500             # the reads' length is their genome's, not 30 times it
    got = pp_sketchlib.queryDatabase(db, db, names, names, KMERS, random_correct=False)
    ref = str(tmp_path / "model" / "model")
    sketchdb.save_npz(ref, names, KMERS, words, 16, 14, lengths=lengths)
    want = pp_sketchlib.queryDatabase(ref, ref, names, names, KMERS, random_correct=False)
    assert got.shape == (3, 2) and np.array_equal(got, want)
    assert got[0, 0] < got[1, 0]                             # rows (reads, own), (reads, far), (own, far)
    # the same three through the resident form
    rdb, stats, _ = sketching.sketch_to_db(names, files, KMERS, 1024, min_count=3)
    assert stats[:, 0].tolist() == lengths.tolist()
    mdb = engine.SketchDB(words, 16, 14, device=0)
    table = synth.random_match_table(KMERS, genome_length=float(lengths.mean()))
    assert torch.equal(engine.dist(rdb, None, KMERS, table)[0], engine.dist(mdb, None, KMERS, table)[0])
    rdb.close()
    mdb.close()
    # without a minimum count the reads are refused and nothing is written
    with pytest.raises(ValueError, match="looks like FASTQ.*minimum k-mer count of 1 or more"):
        pp_sketchlib.constructDatabase(str(tmp_path / "no" / "no"), names, files, KMERS, 1024)
    assert not os.path.exists(str(tmp_path / "no"))
