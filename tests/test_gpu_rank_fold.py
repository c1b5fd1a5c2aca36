"""The folded pair of coded copies (PPK_CODING_FOLD, option "rank_fold"): every bin value that exactly one
sample holds at its (k, bin) position is folded into two reserved codes, 0 on the ref side and 1 on the query side, and
the values with at least two holders get the codes 2 + rank in both.  A triangular self job compares two different
samples, so the bits must be those of the 14 raw planes, from as few as 8 planes.

Settings as in tests/test_gpu_rank_planes.py: s = 1024, five k, option "ksplit" 0 (whole tiles), the random-match table
on.  "Equal" is torch.equal on the distances and on n_failed: "rank_fold" 1 (or 2) against "rank_planes" 0 (the raw
planes) and against "rank_fold" 0 (the injective copy).

Populations: 450 related genomes + 250 of random bins hold up to ~400 distinct values per position (10 planes) of
which fewer than 254 have a second holder (8 planes folded).  200 related genomes tiled x 3 hold no single-holder value
anywhere; there folding gains nothing, so those cases create the database with "rank_fold" 2, which builds the pair
whenever its codes fit.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from poppunk_amd import engine, synth
from rank_model import fold_planes_of, n_distinct, n_shared, shared_mask, unslice

pytestmark = pytest.mark.gpu

KMERS = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
TOL = 1e-6          # tests/test_gpu_dist.py: distances against the CPU oracle
K, BLK, BIT = 2, 5, 37      # the position the small cases overwrite


def random_bins(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 1 << 14, size=(n, 5, 1024), dtype=np.uint16)


def set_position(sk, vals, k=K, blk=BLK, bit=BIT):
    """position (k, 64 * blk + bit) of sample i gets the 14-bit value vals[i] (as overwrite() in test_gpu_rank_short)"""
    vals = np.asarray(vals, dtype=np.uint64)
    assert vals.shape == (len(sk),) and vals.max() < (1 << 14)
    bit = np.uint64(bit)
    for b in range(14):
        w = sk[:, k, blk * 14 + b]
        sk[:, k, blk * 14 + b] = (w & ~(np.uint64(1) << bit)) | (((vals >> np.uint64(b)) & np.uint64(1)) << bit)


@pytest.fixture(scope="module")
def tbl1():
    return synth.random_match_table(KMERS)


@pytest.fixture(scope="module")
def sk700():
    """the population of tests/test_gpu_rank_planes.py: 450 related genomes, a copy of genome 3 and 249 of random bins"""
    sk = np.concatenate([synth.make_sketches(450, KMERS)[0], synth.bitslice(random_bins(250, 5), 14)])
    sk[450] = sk[3]
    return sk


@pytest.fixture(scope="module")
def bins700(sk700):
    return unslice(sk700)


@pytest.fixture(scope="module")
def sk600():
    """200 related genomes x 3: every value has at least three holders"""
    return np.ascontiguousarray(np.tile(synth.make_sketches(200, KMERS)[0], (3, 1, 1)))


@pytest.fixture(scope="module")
def pos600(sk600):
    """the values of the 600 genomes at the position the cases overwrite"""
    vals = unslice(sk600[:, K:K + 1, BLK * 14:(BLK + 1) * 14])[:, 0, BIT].astype(np.uint64)
    assert vals.max() < 16000        # (the cases put their new values at 16000 and above)
    return vals


class Run:
    def __init__(self, out, failed, db):
        self.out, self.failed = out.clone(), failed.clone()
        self.rank_planes, self.fold_planes = db.rank_planes, db.fold_planes
        self.fold_blocks = db.fold_block_planes() if self.fold_planes else None


def run(ppk_option, sk, tbl, rank=1, fold=1, clusters=None, against_itself=False, **band):
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", rank)
    ppk_option("rank_fold", fold)
    db = engine.SketchDB(sk, 16, 14, clusters=clusters)
    try:
        out, failed = engine.dist(db, db if against_itself else None, KMERS, tbl, **band)
        torch.cuda.synchronize()
        return Run(out, failed, db)
    finally:
        db.close()


def same(a, b):
    return torch.equal(a.out, b.out) and torch.equal(a.failed, b.failed)


def three_ways(ppk_option, sk, tbl, **kw):
    """folded, injective and raw: the same bits"""
    got = run(ppk_option, sk, tbl, 1, 1, **kw)
    inj = run(ppk_option, sk, tbl, 1, 0, **kw)
    raw = run(ppk_option, sk, tbl, 0, 1, **kw)
    assert (got.rank_planes, got.fold_planes) == (10, 8)
    assert (inj.rank_planes, inj.fold_planes) == (10, 0)
    assert (raw.rank_planes, raw.fold_planes) == (0, 0)
    assert same(got, raw) and same(inj, raw)
    return got


# ---- folding decides ---------------------------------------------------------------------------------------------------

def test_fold_8_planes_where_ranks_take_10_and_oracle(ppk_option, sk700, bins700, tbl1):
    """700 genomes: full, diagonal, half and strip tiles"""
    assert 256 < int(n_distinct(bins700).max()) <= 1024
    p, want = fold_planes_of(bins700)
    assert p == 8
    got = three_ways(ppk_option, sk700, tbl1)
    assert np.array_equal(got.fold_blocks, want)
    ref, rf = oracle.query(sk700, None, KMERS, 16, 14, tbl1, threads=4)
    assert int(got.failed.item()) == rf and rf > 0          # the random genomes' fits fail
    assert np.abs(got.out.cpu().numpy() - ref).max() <= TOL


def test_fold_band(ppk_option, sk700, tbl1):
    three_ways(ppk_option, sk700, tbl1, q_begin=100, q_end=600)


def test_fold_three_clusters(ppk_option, sk700):
    rng = np.random.Generator(np.random.PCG64(11))
    tbl = synth.random_match_table(KMERS, n_clu=3)
    tbl = (tbl * rng.uniform(0.5, 3.0, size=tbl.shape)).astype(np.float32)
    clu = (np.arange(len(sk700)) % 3).astype(np.uint16)
    three_ways(ppk_option, sk700, tbl, clusters=clu)


def test_fold_off_at_launch_reads_the_raw_planes(ppk_option, sk700, tbl1):
    """a database that holds the pair alone, "rank_fold" 0 when the job is launched"""
    raw = run(ppk_option, sk700, tbl1, 0, 1)
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", 1)
    ppk_option("rank_fold", 1)
    db = engine.SketchDB(sk700, 16, 14)
    try:
        assert db.fold_planes == 8
        ppk_option("rank_fold", 0)
        out, failed = engine.dist(db, None, KMERS, tbl1)
        torch.cuda.synchronize()
        assert torch.equal(out, raw.out) and torch.equal(failed, raw.failed)
    finally:
        db.close()


# ---- the two codes -----------------------------------------------------------------------------------------------------

# new values per sample at the overwritten position.  Samples 5 and 9 share the first diagonal tile (and one 32-query
# tile); 5 and 590 meet in a full tile or the strip.  A kernel given the same copy on both sides would count one match
# too many for two single holders; a builder that took "two holders" for single would lose their one match.
PLACEMENTS = {
    "one_single": {5: 16000},
    "two_singles_one_tile": {5: 16000, 9: 16001},
    "two_singles_far_apart": {5: 16000, 590: 16001},
    "one_pair_one_tile": {5: 16000, 9: 16000},
    "one_pair_far_apart": {5: 16000, 590: 16000},
    "two_pairs_crossed": {5: 16000, 590: 16000, 9: 16001, 300: 16001},
    "pair_and_singles": {5: 16000, 9: 16000, 6: 16001, 590: 16002},
}


@pytest.mark.parametrize("name", sorted(PLACEMENTS))
def test_single_holders_and_pairs(ppk_option, sk600, pos600, tbl1, name):
    sk, vals = sk600.copy(), pos600.copy()
    for smp, v in PLACEMENTS[name].items():
        vals[smp] = v
    set_position(sk, vals)
    got = run(ppk_option, sk, tbl1, 1, 2)
    raw = run(ppk_option, sk, tbl1, 0, 2)
    assert got.fold_planes == 8 and got.rank_planes == 8 and raw.fold_planes == 0
    assert same(got, raw)


def test_no_single_holder_anywhere(ppk_option, sk600, tbl1):
    got = run(ppk_option, sk600, tbl1, 1, 2)
    raw = run(ppk_option, sk600, tbl1, 0, 2)
    assert got.fold_planes == 8 and same(got, raw)


# ---- thresholds of E ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e,planes,block", [(128, 8, 7), (129, 8, 8), (256, 8, 8), (257, 10, 9)])
def test_thresholds_of_e(ppk_option, sk600, tbl1, e, planes, block):
    """one position holds s = e - 2 values with two or three holders each and three single-holder values: E = e there,
    far fewer codes everywhere else"""
    s = e - 2
    vals = np.empty(600, dtype=np.uint64)
    vals[:3] = [16000, 16001, 16002]
    vals[3:] = (np.arange(597) % s) * 3 + 1
    sk = sk600.copy()
    set_position(sk, vals)
    bins = unslice(sk)
    assert int(n_shared(bins)[K, 64 * BLK + BIT]) == s and int(n_distinct(bins)[K, 64 * BLK + BIT]) == s + 3
    p, want = fold_planes_of(bins)
    assert p == planes and want[K, BLK] == block and int((want == planes - 1).sum()) == want.size - (block == planes)
    got = run(ppk_option, sk, tbl1, 1, 2)
    raw = run(ppk_option, sk, tbl1, 0, 2)
    assert got.fold_planes == planes and np.array_equal(got.fold_blocks, want)
    assert same(got, raw)


def test_gain_decides_under_the_default(ppk_option, sk600, tbl1):
    """ "rank_fold" 1 builds the pair only where it compares fewer planes.  E = 128, D = 129: block (2, 5) is short
    folded and full injective, one plane fewer.  E = 129, D = 130: full either way, no pair."""
    for e, folded in ((128, True), (129, False)):
        vals = np.empty(600, dtype=np.uint64)
        vals[:3] = [16000, 16001, 16002]
        vals[3:] = (np.arange(597) % (e - 2)) * 3 + 1
        sk = sk600.copy()
        set_position(sk, vals)
        got = run(ppk_option, sk, tbl1, 1, 1)
        raw = run(ppk_option, sk, tbl1, 0, 1)
        assert got.rank_planes == 8 and got.fold_planes == (8 if folded else 0)
        assert same(got, raw)


# ---- the code builder --------------------------------------------------------------------------------------------------

def test_code_builder_against_numpy(ppk_option, sk700, bins700):
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", 1)
    ppk_option("rank_fold", 1)
    db = engine.SketchDB(sk700, 16, 14)
    try:
        assert db.fold_planes == 8 and db.rank_planes == 10
        ref, qry = db.fold_codes(0), db.fold_codes(1)
        inj = db.rank_codes()          # (built on demand: the database holds the pair alone)
    finally:
        db.close()
    assert ref.shape == bins700.shape and qry.shape == bins700.shape
    assert int(ref.max()) < (1 << 8) and int(qry.max()) < (1 << 8)
    shared = shared_mask(bins700)
    assert shared.any() and not shared.all()
    # single holders: 0 on the ref side, 1 on the query side
    assert not ref[~shared].any() and (qry[~shared] == 1).all()
    # shared values: one code >= 2 on both sides, injective among the shared values of a position, 2 + rank
    assert np.array_equal(ref[shared], qry[shared]) and int(ref[shared].min()) == 2
    vals = np.where(shared, bins700, 0xffff).astype(np.uint32)
    codes = np.where(shared, ref, 0xffff).astype(np.uint32)
    nv = n_distinct(vals)
    assert np.array_equal(n_distinct(vals << 16 | codes), nv) and np.array_equal(n_distinct(codes), nv)
    assert np.array_equal(np.where(shared, ref, 1).max(axis=0), n_shared(bins700) + 1)
    # the injective copy, asked for afterwards, is what tests/test_gpu_rank_planes.py pins
    assert int(inj.max()) < (1 << 10)
    nb = n_distinct(bins700)
    assert np.array_equal(n_distinct(bins700.astype(np.uint32) << 16 | inj), nb) and np.array_equal(n_distinct(inj), nb)


# ---- the same handle as the query --------------------------------------------------------------------------------------

def test_handle_against_itself_does_not_read_the_pair(ppk_option, sk700, tbl1):
    """the rectangular job has the pairs (r, r), where a single-holder value matches itself"""
    got = run(ppk_option, sk700, tbl1, 1, 1, against_itself=True)
    raw = run(ppk_option, sk700, tbl1, 0, 1, against_itself=True)
    assert got.fold_planes == 8 and raw.fold_planes == 0
    assert same(got, raw)
    n = len(sk700)
    diag = got.out.view(n, n, 2)[torch.arange(n), torch.arange(n)]
    assert float(diag.abs().max()) <= TOL


def test_handle_against_itself_after_the_injective_copy_was_built(ppk_option, sk700, tbl1):
    raw = run(ppk_option, sk700, tbl1, 0, 1, against_itself=True)
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", 1)
    ppk_option("rank_fold", 1)
    db = engine.SketchDB(sk700, 16, 14)
    try:
        assert db.fold_planes == 8
        db.rank_codes()
        out, failed = engine.dist(db, db, KMERS, tbl1)
        torch.cuda.synchronize()
        assert torch.equal(out, raw.out) and torch.equal(failed, raw.failed)
    finally:
        db.close()


# ---- no gain, no change ------------------------------------------------------------------------------------------------

def test_no_gain_no_pair(ppk_option):
    sk = synth.make_sketches(300, KMERS)[0]
    ppk_option("ksplit", 0)
    ppk_option("rank_planes", 1)
    ppk_option("rank_fold", 1)
    db = engine.SketchDB(sk, 16, 14)
    try:
        assert db.fold_planes == 0 and db.rank_planes == 8
        codes = db.rank_codes()
        with pytest.raises(RuntimeError):
            db.fold_block_planes()
    finally:
        db.close()
    vals = unslice(sk)
    assert codes.shape == vals.shape and int(codes.max()) < (1 << 8)
    nv = n_distinct(vals)
    assert np.array_equal(n_distinct(vals.astype(np.uint32) << 16 | codes), nv) and np.array_equal(n_distinct(codes), nv)
