"""Host side of the pair-list path: rows <-> pairs in exact integers, and the training-row draw
whose memory does not grow with the matrix.  No GPU."""
import tracemalloc

import numpy as np
import pytest

from poppunk_amd import engine, models, utils


def _self_rows(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


@pytest.mark.parametrize("n", [2, 3, 5, 65])
def test_rows_to_pairs_inverts_the_self_row_order(n):
    names = [str(k) for k in range(n)]
    # iterDistRows names a row (ref j, query i), i < j; the edge form is (i, j)
    want = [(int(b), int(a)) for a, b in utils.iterDistRows(names, names, self=True)]
    assert want == _self_rows(n)
    got = engine.rows_to_pairs(np.arange(len(want)), n)
    assert got.dtype == np.int64 and got.shape == (len(want), 2)
    assert [tuple(r) for r in got.tolist()] == want


@pytest.mark.parametrize("n_ref,n_qry", [(3, 2), (130, 7)])
def test_rows_to_pairs_inverts_the_ref_query_row_order(n_ref, n_qry):
    refs, qrys = ["r%d" % k for k in range(n_ref)], ["q%d" % k for k in range(n_qry)]
    order = list(utils.iterDistRows(refs, qrys, self=False))
    assert len(order) == n_ref * n_qry
    got = engine.rows_to_pairs(np.arange(len(order)), n_ref, n_qry)
    # edge form: (ref r, n_ref + query q), as generate_tuples numbers a ref x query row (src/boundary.cpp:113-114)
    names = refs + qrys
    pairs = [(names[a], names[b]) for a, b in got.tolist()]
    assert all(0 <= a < n_ref <= b < n_ref + n_qry for a, b in got.tolist())
    assert [tuple(sorted(p)) for p in pairs] == [tuple(sorted(p)) for p in order]


@pytest.mark.parametrize("n", [3_000_000, 40_000_000])
def test_rows_to_pairs_round_trips_at_large_n(n):
    """Beyond 2^52 the double square root rounds: the integer fix-up has to carry the result."""
    n_rows = n * (n - 1) // 2

    def start(i):
        return i * n - i * (i + 1) // 2          # Python integers: the forward condensed formula
    rows = []
    for i in (0, n // 2, n - 2):
        rows += [start(i), start(i + 1) - 1]
    rng = np.random.default_rng(n)
    rows += rng.integers(0, n_rows, size=10000).tolist()
    got = engine.rows_to_pairs(np.asarray(rows, dtype=np.int64), n)
    for row, (i, j) in zip(rows, got.tolist()):
        assert 0 <= i < j < n
        assert start(i) + (j - i - 1) == row
    with pytest.raises(ValueError):
        engine.rows_to_pairs([n_rows], n)
    with pytest.raises(ValueError):
        engine.rows_to_pairs([-1], n)


def test_sample_rows_is_the_matrix_routes_draw_where_that_fits():
    got = models.sample_rows(44850, 5000, 42)
    assert np.array_equal(got, models.DBSCANModel.subsample_index(44850, 5000, 42))
    assert got.shape == (5000,)
    assert models.sample_rows(5000, 5000, 42) is None
    assert models.sample_rows(10, 100000, 42) is None
    assert models.sample_rows(5_000_000_000, 5_000_000_000, 42) is None


def test_sample_rows_of_a_matrix_that_cannot_exist():
    n_rows = 4_999_950_000                       # 100 000 genomes
    tracemalloc.start()
    try:
        got = models.sample_rows(n_rows, 100000, 42)
        _, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    assert peak < 64 << 20, peak
    assert got.dtype == np.int64 and got.shape == (100000,)
    assert got.min() >= 0 and got.max() < n_rows
    assert np.unique(got).size == 100000
    assert np.array_equal(got, models.sample_rows(n_rows, 100000, 42))
    assert not np.array_equal(got, models.sample_rows(n_rows, 100000, 43))
