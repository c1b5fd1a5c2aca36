"""The arithmetic of the two-holder pair (option "rank_fold2"), on the CPU: tests/rank_fold2_model.py against brute
force.  What the device must reproduce is stated here once: with the values of exactly two holders coded like
single-holder ones, the compare of (ref copy of r, query copy of q), r > q, plus the events of (r, q, k) is the true
match count -- for every pair and k; the codes of a position span E2 = S3 + 2 values; the buckets hold every event once;
the caps and the plane-sum rule decide what ppk_db_create builds.  `choice` asks the numpy model AND the library
(ppk_choose_coding, no device touched) and returns what both say (tests/coding_choice.py)."""
import numpy as np

from coding_choice import counts_layout, plan
from coding_choice import fold2_choice as choice
from rank_fold2_model import (MAX_PER_PAIR, SLOTS, block_counts, buckets_of, counts_of, events_of, fold2_codes_of,
                              match_counts, per_pair_max)
from rank_model import fold_codes_of, n_distinct, n_shared
from rank_sort_model import order_of, planted_e2, position_e2, spread_targets, stream_planes


def population(n=90, nk=3, nbins=128, values=700, seed=5):
    """few values per position: holders of 1, 2, 3 and more all occur, and some pairs collide more than once"""
    rng = np.random.Generator(np.random.PCG64(seed))
    bins = rng.integers(0, values, size=(n, nk, nbins)).astype(np.uint16)
    bins[7, :, 1::2] = 15000                 # a pair that alone holds one value at each of the 64 odd positions ...
    bins[40] = bins[7]
    bins[40, :, ::2] = 16000                 # ... and shares none of the even ones
    return bins


def test_counts_against_brute_force():
    bins = population()
    d, s, s3, t = counts_of(bins)
    assert np.array_equal(d, n_distinct(bins)) and np.array_equal(s, n_shared(bins))
    for k, b in [(0, 0), (1, 17), (2, 127)]:
        held = np.unique(bins[:, k, b], return_counts=True)[1]
        assert (d[k, b], s[k, b], s3[k, b], t[k, b]) == (len(held), (held >= 2).sum(), (held >= 3).sum(), (held == 2).sum())
    assert t.min() >= 0 and t.max() > 0 and s3.max() > 0


def test_codes_span_e2_and_keep_three_holder_values_apart():
    bins = population()
    ref, qry = fold2_codes_of(bins)
    _, _, s3, _ = counts_of(bins)
    assert np.array_equal(np.maximum(ref, qry).max(axis=0) + 1, np.where(s3 > 0, s3 + 2, 2))
    coded = ref >= 2
    assert np.array_equal(ref[coded], qry[coded]) and (ref[~coded] == 0).all() and (qry[~coded] == 1).all()
    # coded values: equal codes exactly where the values are equal
    k, b = 1, 17
    col, c = bins[:, k, b], ref[:, k, b]
    m = c >= 2
    assert np.array_equal(col[m][:, None] == col[m][None, :], c[m][:, None] == c[m][None, :])


def test_compare_plus_events_is_the_true_count():
    bins = population()
    n, nk = bins.shape[:2]
    true = match_counts(bins, bins)
    ref, qry = fold2_codes_of(bins)
    seen = match_counts(ref, qry)                       # [r, q, k]
    owed = np.zeros_like(seen)
    ev = events_of(bins)
    np.add.at(owed, (ev[:, 0], ev[:, 1], ev[:, 2]), 1)
    tri = np.tril(np.ones((n, n), dtype=bool), -1)      # r > q
    assert (ev[:, 0] > ev[:, 1]).all() and owed.max() > 1
    assert np.array_equal((seen + owed)[tri], true[tri])
    assert not np.array_equal(seen[tri], true[tri])
    # the folded pair of one step earlier needs no events
    fr, fq = fold_codes_of(bins)
    assert np.array_equal(match_counts(fr, fq)[tri], true[tri])


def test_buckets_hold_every_event_once():
    bins = population(n=300, nk=2, nbins=64, values=3000)
    ev = events_of(bins)
    off, packed = buckets_of(ev, 300)
    assert len(off) == 16 * 2 + 1 and off[-1] == len(ev) == len(packed)
    back = []
    for b in range(len(off) - 1):
        for e in packed[off[b]:off[b + 1]].astype(np.int64):
            back.append(((b % 2) * 256 + (e & 255), (b // 2) * 32 + ((e >> 8) & 31), e >> 13))
    assert sorted(back) == sorted(map(tuple, ev))
    assert (ev[:, 0] >= 256).any() and (ev[:, 1] >= 256).any()      # strip samples on either side


def test_choice_rule_and_caps():
    bd = np.full((5, 16), 300, dtype=np.int64)       # 10 planes, short
    be = np.full((5, 16), 140, dtype=np.int64)       # 8 planes, full
    be2 = np.full((5, 16), 80, dtype=np.int64)       # 8 planes, short
    big, small = 10000, 2100
    assert choice(bd, be, be2, 100, 3, big) == "fold2"
    assert choice(bd, be, be2, 100, 3, small) == "fold"                       # under four rounds of tiles
    assert choice(bd, be, be2, 100, 3, small, rank_fold2=2) == "fold2"
    assert choice(bd, be, be2, 100, 3, big, rank_fold2=0) == "fold"
    assert choice(bd, be, be2, 100, 3, big, rank_fold=0) == "rank"
    assert choice(bd, be, be2, 100, 3, big, rank_fold=0, rank_fold2=2) == "fold2"
    assert choice(bd, be, be, 100, 3, big) == "fold"                           # no plane gained over the folded pair
    assert choice(bd, be, np.full((5, 16), 129), 100, 3, big) == "fold"
    for forced in (1, 2):
        assert choice(bd, be, be2, SLOTS, MAX_PER_PAIR, big, rank_fold2=forced) == "fold2"
        assert choice(bd, be, be2, SLOTS + 1, 3, big, rank_fold2=forced) == "fold"
        assert choice(bd, be, be2, 100, MAX_PER_PAIR + 1, big, rank_fold2=forced) == "fold"
        assert choice(np.full((6, 16), 300), np.full((6, 16), 140), np.full((6, 16), 80), 100, 3, big, rank_fold2=forced) == "fold"
        assert choice(bd, be, np.full((5, 16), 257), 100, 3, big, rank_fold2=forced) == "fold"      # E2 past 8 planes


def test_caps_are_what_the_model_counts():
    bins = population()
    assert per_pair_max(events_of(bins)) == 64          # samples 7 and 40: the 64 odd positions of each k
    bd, be, be2, two_max, two_total = block_counts(bins)
    assert two_total == len(events_of(bins)) and two_max == counts_of(bins)[3].max()
    assert choice(bd, be, be2, two_max, 64, len(bins), rank_fold2=2) != "fold2"
    bins[40, :, 1] = 15999                               # one fewer
    assert per_pair_max(events_of(bins)) == 63
    bd, be, be2, two_max, _ = block_counts(bins)
    assert choice(bd, be, be2, two_max, 63, len(bins), rank_fold2=2) == "fold2"


def flag_bits(words, nk, s64):
    """per-k flag words -> bool [nk, s64]"""
    return (words[:nk, None] >> np.arange(s64)[None, :] & 1).astype(bool)


def test_the_library_plans_the_sorted_pair_like_the_model():
    """what the models of the choice cannot say: the slot order, the 7- and 6-plane flags, the stream planes and their
    sum of ppk_choose_coding are rank_sort_model's, sorted and as stored, on a population whose blocks take 8, 7 and 6"""
    targets = spread_targets(2, 192, 140, seed=11, wide=[[(140, 3), (100, 70)], [(90, 5)]])
    for bins in (population(), planted_e2(430, targets, seed=12)):
        bd, be, be2, two_max, two_total = block_counts(bins)
        e2 = position_e2(bins)
        nk, s64 = bd.shape
        for sort in (1, 0):
            p = plan(counts_layout(bd, be, be2, two_max, two_total, e2), len(bins), nk, s64, rank_fold2=2, fold2_sort=sort)
            order = order_of(e2, bool(sort))
            want = stream_planes(e2, order)
            assert p["first"] == "fold2" and p["try_holder"]
            assert np.array_equal(p["order"], order) and np.array_equal(p["stream"], want) and p["stream_sum"] == want.sum()
            assert np.array_equal(flag_bits(p["seven"], nk, s64), want <= 7) and np.array_equal(flag_bits(p["six"], nk, s64), want <= 6)
            assert not p["seven"][nk:].any() and not p["six"][nk:].any()
            seen = set(want.ravel().tolist()) if sort else seen
    assert seen == {6, 7, 8}      # (the planted population, sorted)
    # nothing but the first coding has an order: the folded pair first leaves every output empty
    p = plan(counts_layout(bd, be, be2, two_max, two_total, e2), len(bins), nk, s64, rank_fold2=0)
    assert p["first"] in ("fold", "rank") and p["stream_sum"] == 0 and not p["order"].any() and not p["try_holder"]
