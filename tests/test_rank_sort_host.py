"""The sorted positions of the two-holder pair (options "fold2_sort", "fold2_min_planes"), on the CPU:
tests/rank_sort_model.py against brute force and against the rule as the issue states it."""
import numpy as np
import pytest

from rank_fold2_model import events_of, fold2_codes_of, match_counts
from rank_sort_model import in_slots, order_of, planted_e2, position_e2, spread_targets, stream_planes


def test_permuted_copies_plus_events_count_every_match():
    """compare of the two copies in slot order, plus the events, is the brute-force count for every pair and k"""
    n, nk, nbins = 40, 3, 128
    targets = np.random.default_rng(5).integers(2, 13, size=(nk, nbins))
    bins = planted_e2(n, targets, seed=6)
    e2 = position_e2(bins)
    assert np.array_equal(e2, targets)
    order = order_of(e2)
    assert not np.array_equal(order, order_of(e2, sort=False))
    ref, qry = fold2_codes_of(bins)
    slotted = match_counts(in_slots(ref, order), in_slots(qry, order))
    ev = events_of(bins)
    assert len(ev) > 50
    got = slotted.copy()
    np.add.at(got, (ev[:, 0], ev[:, 1], ev[:, 2]), 1)
    want = match_counts(bins, bins)
    hi, lo = np.tril_indices(n, -1)
    assert np.array_equal(got[hi, lo], want[hi, lo])
    # (the order matters to neither term: the copies in stored order count the same)
    assert np.array_equal(match_counts(ref, qry)[hi, lo], slotted[hi, lo])


def test_order_is_a_permutation_sorted_descending_with_ties_in_stored_order():
    rng = np.random.default_rng(1)
    e2 = rng.integers(2, 9, size=(4, 256))      # (few values: long runs of ties)
    order = order_of(e2)
    for k in range(4):
        assert np.array_equal(np.sort(order[k]), np.arange(256))
        s = e2[k, order[k]]
        assert (s[1:] <= s[:-1]).all()
        tied = s[1:] == s[:-1]
        assert tied.any() and (order[k, 1:][tied] > order[k, :-1][tied]).all()
    assert np.array_equal(order_of(e2, sort=False), np.tile(np.arange(256), (4, 1)))


def test_planes_never_increase_along_a_sorted_k():
    rng = np.random.default_rng(2)
    e2 = rng.integers(2, 200, size=(5, 1024))
    e2[1] = rng.integers(2, 65, size=1024)
    e2[2] = rng.integers(2, 129, size=1024)
    planes = stream_planes(e2, order_of(e2))
    assert (planes[:, 1:] <= planes[:, :-1]).all()
    assert (planes[1] == 6).all() and set(planes[2]) <= {6, 7} and set(planes[0]) == {6, 7, 8}
    # sorting never compares more planes than the stored order
    assert planes.sum() <= stream_planes(e2, order_of(e2, sort=False)).sum()


@pytest.mark.parametrize("widest,want", [(64, 6), (65, 7), (128, 7), (129, 8)])
def test_thresholds(widest, want):
    e2 = np.full((1, 128), 30)
    e2[0, 77] = widest
    order = order_of(e2)
    assert order[0, 0] == (77 if widest > 30 else 0)
    assert list(stream_planes(e2, order)[0]) == [want, 6]
    assert list(stream_planes(e2, order_of(e2, sort=False))[0]) == [6, want]
    assert list(stream_planes(e2, order, min_planes=7)[0]) == [max(want, 7), 7]
    assert list(stream_planes(e2, order, rank_short=0)[0]) == [8, 8]


def test_flags_are_kept_for_at_most_32_blocks():
    e2 = np.full((2, 64 * 33), 10)
    assert (stream_planes(e2, order_of(e2)) == 8).all()
    assert (stream_planes(e2[:, :64 * 32], order_of(e2[:, :64 * 32])) == 6).all()
