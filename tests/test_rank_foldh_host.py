"""The holder pair (options "rank_foldh", "foldh_holders", "foldh_min_planes") on the CPU: tests/foldh_model.py against
brute force on planted populations and against the rule as the issue states it, and the figures of the benchmark's
database (synth.make_sketches(10000)): H = 64, 163 stream planes, 2 693 184 entries.  `choice` asks the numpy model
AND the library (ppk_choose_holder, no device touched) and returns what both say (tests/coding_choice.py)."""
import numpy as np
import pytest

from coding_choice import counts_layout, holder, plan
from coding_choice import holder_choice as choice
from foldh_model import (LADDER, block_planes, buckets_of, entries_of, foldh_codes_of, held_of, match_counts,
                         max_entries, owed_brute, planted_holders, position_eh, stream_planes)
from rank_sort_model import in_slots, order_of


def planted(n=120, nk=3, nbins=128, h=4, seed=3, top=13):
    kept = np.random.default_rng(seed).integers(0, top, size=(nk, nbins))
    return planted_holders(n, kept, h, seed=seed + 1), kept


def test_copies_in_slot_order_plus_entries_count_every_match():
    h = 4
    bins, kept = planted(h=h)
    eh = position_eh(bins, h)
    assert np.array_equal(eh, kept + 2)
    order = order_of(eh)
    ref, qry = foldh_codes_of(bins, h)
    slotted = match_counts(in_slots(ref, order), in_slots(qry, order))
    ent = entries_of(bins, h)
    assert len(ent) > 200 and ent[:, 3].max() > 1 and (ent[:, 0] > ent[:, 1]).all()
    got = slotted.copy()
    got[ent[:, 0], ent[:, 1], ent[:, 2]] += ent[:, 3]
    want = match_counts(bins, bins)
    hi, lo = np.tril_indices(len(bins), -1)
    assert np.array_equal(got[hi, lo], want[hi, lo])
    # the entries are the brute-force counts, one per (pair, k) that is owed anything
    dense = np.zeros_like(want)
    dense[ent[:, 0], ent[:, 1], ent[:, 2]] = ent[:, 3]
    assert np.array_equal(dense, owed_brute(bins, h)) and len(np.unique(ent[:, :3], axis=0)) == len(ent)
    # at a position both samples hold either a common coded value or a common folded one, never both
    assert np.array_equal(match_counts(ref, qry)[hi, lo] + dense[hi, lo], want[hi, lo])


def test_a_value_with_exactly_h_holders_is_folded_and_one_with_h_plus_one_is_coded():
    for h in (4, 8):
        bins, kept = planted(n=200, h=h, top=5)
        held, (ref, qry) = held_of(bins), foldh_codes_of(bins, h)
        assert (held == h).any() and (held == h + 1).any() and (held == 2).any()
        assert (ref[held <= h] == 0).all() and (qry[held <= h] == 1).all()
        assert (ref[held > h] >= 2).all() and np.array_equal(ref[held > h], qry[held > h])
        # codes are dense per position: 2 .. E_H - 1
        assert np.array_equal(ref.max(axis=0) + 1, np.where(kept > 0, kept + 2, 1))


@pytest.mark.parametrize("widest,want", [(3, 2), (4, 2), (5, 3), (8, 3), (9, 4), (16, 4), (17, None)])
def test_block_planes(widest, want):
    eh = np.full((2, 128), 2)
    eh[1, 77] = widest
    planes = block_planes(eh, order_of(eh))
    if want is None:
        assert planes is None
        assert choice(lambda h: eh, 10 ** 6, 10000, 2, 2, rank_foldh=2) is None
    else:
        assert planes.tolist() == [[2, 2], [want, 2]]      # (sorted: the wide position leads its k)
        assert stream_planes(eh, order_of(eh), min_planes=3).tolist() == [[3, 3], [max(want, 3), 3]]
        assert (stream_planes(eh, order_of(eh), min_planes=4) == 4).all()
        assert (stream_planes(eh, order_of(eh), rank_short=0) == 4).all()


def test_the_ladder_picks_the_smallest_h_that_qualifies():
    # E_H shrinks with H: 40 codes at 4 and 8, 16 at 16 and 32, 4 from 64 on
    def eh_of(h):
        return np.full((5, 1024), 40 if h < 16 else 16 if h < 64 else 4)
    n, fold2_sum = 10000, 490
    assert choice(eh_of, fold2_sum, n, 5, 16) == 64                 # at 16: 4 planes x 80 = 320 > 0.6 x 490; at 64: 160
    assert choice(eh_of, 534, n, 5, 16) == 16                       # 320 <= 0.6 x 534 = 320.4: just inside
    assert choice(eh_of, 533, n, 5, 16) == 64                       # 320 > 319.8: just past, the next rung that pays
    assert choice(eh_of, 267, n, 5, 16) == 64                       # 160 <= 160.2
    assert choice(eh_of, 266, n, 5, 16) is None                     # 160 > 159.6: no rung pays
    assert choice(eh_of, fold2_sum, n, 5, 16, rank_foldh=2) == 16   # whenever the blocks fit
    assert choice(eh_of, fold2_sum, n, 5, 16, rank_foldh=0) is None
    assert choice(eh_of, fold2_sum, n, 5, 16, foldh_holders=8) is None and choice(eh_of, fold2_sum, n, 5, 16, foldh_holders=128) == 128
    assert choice(eh_of, fold2_sum, 2100, 5, 16) is None            # under four rounds of tiles
    assert choice(eh_of, fold2_sum, 2100, 5, 16, rank_foldh=2) == 16
    assert choice(lambda h: np.full((6, 1024), 4), fold2_sum, n, 6, 16, rank_foldh=2) is None      # six k
    assert choice(lambda h: np.full((5, 64 * 33), 4), 10 ** 6, n, 5, 33, rank_foldh=2) is None     # 33 blocks per k
    assert LADDER == (4, 8, 16, 32, 64, 128, 256)


def test_the_cap_on_the_entries():
    """a database planted one entry past a sixteenth of its (pair, k) is refused, one just inside is accepted"""
    n, nk, nbins = 120, 1, 512
    cap = max_entries(n, nk)
    assert cap == n * (n - 1) // 2 * nk // 16 == 446 and max_entries(n, nk, 2) == n * (n - 1) // 2 * nk
    hi, lo = np.tril_indices(n, -1)
    bins = (1000 + np.arange(n))[:, None, None] + np.zeros((1, nk, nbins), dtype=np.int64)
    for p in range(cap + 1):      # one two-holder value per position, each on a pair of its own
        bins[[hi[7 * p], lo[7 * p]], 0, p] = 7
    past = entries_of(bins.astype(np.uint16), 4)
    assert len(past) == cap + 1 and (past[:, 3] == 1).all() and not len(past) <= cap
    assert len(past) <= max_entries(n, nk, 2)                    # "rank_foldh" 2 takes it
    bins[hi[0], 0, 0] = 8
    assert len(entries_of(bins.astype(np.uint16), 4)) == cap


def test_two_identical_samples_are_owed_every_bin():
    n, nk, s64 = 40, 2, 16
    bins = (np.arange(n)[:, None, None] * 300 + np.arange(nk * 64 * s64).reshape(1, nk, -1) % 290).astype(np.uint16)
    bins[31] = bins[6]
    ent = entries_of(bins, 4)
    assert ent.tolist() == [[31, 6, 0, 1024], [31, 6, 1, 1024]]
    off, packed = buckets_of(ent, n)
    assert (packed >> 16).tolist() == [1024, 1024] and off[-1] == 2      # 12 bits hold it


def test_buckets_hold_the_entries():
    bins, _ = planted(n=300, nk=2, nbins=64, h=4, top=4)
    ent = entries_of(bins, 4)
    off, packed = buckets_of(ent, 300)
    back = []
    for b in range(len(off) - 1):
        for e in packed[off[b]:off[b + 1]].astype(np.int64):
            back.append(((b % 2) * 256 + (e & 255), (b // 2) * 32 + ((e >> 8) & 31), (e >> 13) & 7, e >> 16))
    assert sorted(back) == sorted(map(tuple, ent)) and (ent[:, 0] >= 256).any()


def test_the_benchmark_database():
    """synth.make_sketches(10000): the rule lands on H = 64 with 163 stream planes -- 2 in 77 blocks, 3 in 3 -- against
    the two-holder pair's 490, and 2 693 184 entries of which 1 463 328 carry count 1 and 1 223 377 more than 63"""
    from poppunk_amd import synth
    from rank_fold2_model import counts_of
    from rank_model import block_max, unslice
    from rank_sort_model import stream_planes as fold2_stream_planes
    n = 10000
    bins = unslice(synth.make_sketches(n)[0])
    d, s, s3, two = counts_of(bins)
    e2 = s3 + 2                                          # (rank_sort_model.position_e2)
    fold2_sum = int(fold2_stream_planes(e2, order_of(e2)).sum())
    assert fold2_sum == 490
    # the library's plan from the same figures: the two-holder pair first, its order and its 490 planes, the holder
    # pair to be tried beside it
    p = plan(counts_layout(block_max(d), block_max(s + 2), block_max(e2), int(two.max()), int(two.sum()), e2), n, 5, 16)
    assert (p["first"], p["fallback"], p["stream_sum"], p["try_holder"]) == ("fold2", "fold", 490, True)
    assert np.array_equal(p["order"], order_of(e2)) and np.array_equal(p["stream"], fold2_stream_planes(e2, order_of(e2)))
    cache = {}

    def eh_of(h):
        if h not in cache:
            cache[h] = position_eh(bins, h)
        return cache[h]
    assert choice(eh_of, fold2_sum, n, 5, 16) == 64
    assert eh_of(32).max() == 77 and eh_of(64).max() == 5
    planes = block_planes(eh_of(64), order_of(eh_of(64)))
    assert int(planes.sum()) == 163
    got_h, got_order, got_planes, got_cap = holder(eh_of, p["stream_sum"], n, 5, 16, most_shared=int(s.max()))
    assert got_h == 64 and int(got_planes.sum()) == 163 and np.array_equal(got_planes, planes)
    assert np.array_equal(got_order, order_of(eh_of(64))) and got_cap == max_entries(n, 5)
    assert [np.bincount(row, minlength=5)[2:].tolist() for row in planes] == [[16, 0, 0], [16, 0, 0], [15, 1, 0], [15, 1, 0], [15, 1, 0]]
    ent = entries_of(bins, 64)
    assert len(ent) == 2693184 <= max_entries(n, 5)
    assert int((ent[:, 3] == 1).sum()) == 1463328 and int((ent[:, 3] > 63).sum()) == 1223377 and int(ent[:, 3].max()) == 377
