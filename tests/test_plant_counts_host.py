"""CPU tests of tests/plant_counts.py: planted match-count vectors against oracle.match_counts, exact_fit against
oracle.fit on every lattice the GPU tests plant (tests/test_gpu_fit_lattice.py), the width of every tripwire band
tests/test_gpu_tripwire_edges.py threads a boundary through, and its two BGMM models against the numpy restatement of
tests/test_bgmm_host.py.  The largest |oracle fp64 - exact| found here, before rounding, is plant_counts.FP64_ERR."""
import math

import numpy as np
import pytest

import plant_counts as pc
from oracle import oracle
from poppunk_amd import synth
from rank_fold2_model import events_of, per_pair_max
from test_bgmm_host import restated


def population(n, kmers, s64, bbits, seed=7):
    sk = synth.make_sketches(n, kmers, sketchsize64=s64, bbits=bbits, cluster_size=10, seed=seed)[0]
    return oracle.deslice(sk, s64, bbits).astype(np.uint16)


@pytest.mark.parametrize("s64,bbits,nk", [(16, 14, 5), (156, 14, 6), (20, 10, 4)])
def test_planted_vectors_equal_the_oracle_counts(s64, bbits, nk):
    kmers = pc.kmers_of(nk)
    nbins = 64 * s64
    bins = population(24, kmers, s64, bbits)
    before = bins.copy()
    mid = pc.falling(kmers, nbins)
    ends = (0, 63, nbins - 64, nbins - 1)          # first and last bin of the first and last block
    targets = [(3, 20, mid), (11, 4, (nbins,) * nk), (5, 6, (0,) * nk), (23, 0, tuple(reversed(mid))),
               (8, 15, tuple(2 + i for i in range(nk)))]
    for q, r, _ in targets[:2]:          # no match at the ends: they qualify for what is planted first
        bins[r][:, ends] = bins[q][:, ends] ^ 1
    before = bins.copy()
    touched = pc.plant(bins, targets, bbits=bbits, events=[4, 0, 0, 1, 2], seed=5, first=ends)
    counts = oracle.match_counts(synth.bitslice(bins, bbits), None, s64, bbits)
    was = oracle.match_counts(synth.bitslice(before, bbits), None, s64, bbits)
    n = len(bins)
    row = lambda i, j: i * n - i * (i + 1) // 2 + (j - i - 1)
    for q, r, vec in targets:
        assert tuple(counts[row(min(q, r), max(q, r))]) == tuple(vec)
    planted = {s for q, r, _ in targets for s in (q, r)}
    rest = [row(i, j) for i in range(n) for j in range(i + 1, n) if i not in planted and j not in planted]
    assert np.array_equal(counts[rest], was[rest])
    for rows in touched[:2]:          # events at the four ends; matches added there
        for pos in rows:
            assert set(ends) <= set(pos.tolist())
            assert len(np.unique(pos // 64)) > s64 // 2          # drawn over the blocks, not the first ones
    assert (bins < (1 << bbits)).all()


def test_planting_is_seeded_and_refuses_what_it_cannot_do():
    kmers = pc.kmers_of(5)
    bins = population(12, kmers, 2, 14)
    a, b = bins.copy(), bins.copy()
    t = [(0, 1, (40, 30, 20, 10, 5))]
    pc.plant(a, t, seed=3)
    pc.plant(b, t, seed=3)
    assert np.array_equal(a, b)
    pc.plant(b, t, seed=3)          # already there: nothing to do
    assert np.array_equal(a, b)
    c = bins.copy()
    pc.plant(c, t, seed=4)
    assert not np.array_equal(a, c)
    with pytest.raises(ValueError, match="distinct"):
        pc.plant(bins.copy(), [(0, 1, (1,) * 5), (1, 2, (1,) * 5)])
    with pytest.raises(ValueError, match="does not fit"):
        pc.plant(bins.copy(), [(0, 1, (129,) * 5)])
    with pytest.raises(ValueError, match="may be rewritten"):
        pc.plant(bins.copy(), [(0, 1, (100,) * 5)], avoid=np.ones((5, 128), dtype=bool))


def test_keep_coded_leaves_the_events_of_a_tripled_population_alone():
    """the population of tests/test_gpu_tripwire_edges.py in small: every natural value has three holders or more; after
    planting under keep_coded the events are those from before plus the planted ones, `events` per (target, k)"""
    kmers = pc.kmers_of(5)
    base = population(30, kmers, 16, 14)
    bins = np.tile(base, (3, 1, 1))
    bins[[2, 50], 1, 7] = 16383          # an event that is there before
    assert (bins[[2, 50], 1, 7][:, None] != np.delete(bins[:, 1, 7], [2, 50])[None, :]).all()
    before = set(map(tuple, events_of(bins)))
    targets = [(1, 41, pc.FALLING), (88, 17, pc.FALLING), (63, 64, pc.FALLING)]          # pairs across clusters
    pc.plant(bins, targets, events=[2, 0, 1], seed=9, keep_coded=True)
    ev = events_of(bins)
    after = set(map(tuple, ev))
    new = [e for e in map(tuple, ev) if e not in before]
    assert before <= after
    assert sorted(new) == sorted([(41, 1, k) for k in range(5)] * 2 + [(64, 63, k) for k in range(5)])
    assert per_pair_max(ev) == 2


# ---- exact_fit against the oracle's fp64 ----------------------------------------------------------------------------
def fp64_fit(vector, kmers, nbins, bbits, rtab_row, collision_adjust, fit_skip):
    """a4 - a6 of oracle/ppk_oracle.c operation for operation in Python floats (fp64, the same libm): the Jaccards the
    oracle's fit is given, and its core and accessory distances BEFORE they are rounded to float32"""
    expected = nbins >> bbits
    jac = []
    for i, same in enumerate(vector):
        inter = int(same)
        if collision_adjust and expected:
            inter = max(inter - expected, 0) * nbins // (nbins - expected)
        obs = float(inter) / float(nbins)
        expd = float(np.float32(rtab_row[i])) if rtab_row is not None else 0.0
        jac.append(((obs - expd) if obs > expd else 0.0) / (1.0 - expd))
    tol = 5.0 / float(nbins)
    n = 0
    sx = sxx = sy = sxy = 0.0
    for i, j in enumerate(jac):
        if j < tol:
            if fit_skip:
                continue
            break
        x, y = float(kmers[i]), math.log(j)
        sx += x
        sxx += x * x
        sy += y
        sxy += x * y
        n += 1
    if n < 2:
        return jac, 0.0, 0.0, True
    dn = float(n)
    slope = (dn * sxy - sx * sy) / (dn * sxx - sx * sx)
    intercept = (sy - slope * sx) / dn
    return jac, (1.0 - math.exp(slope) if slope < 0 else 0.0), (1.0 - math.exp(intercept) if intercept < 0 else 0.0), False


def within_one_ulp(got, ref):
    """1 float32 ulp of the reference.  Where the exact value is 0 and the oracle's is not -- the constant vector, whose
    slope is a residue of fp64 rounding in n sxy - sx sy -- no float32 ulp measures the difference: the residue is an
    fp64 error like any other and is held to FP64_ERR, the figure this file records"""
    if ref == 0:
        return abs(float(got)) <= pc.FP64_ERR
    return abs(float(got) - float(ref)) <= pc.ulp32(ref)


def test_exact_fit_against_the_oracle_on_every_lattice():
    worst = 0.0
    smallest_margin = np.inf
    n_points = 0
    try:
        for s64, bbits, nk, adjust in pc.LATTICE_SHAPES:
            kmers = pc.kmers_of(nk)
            nbins = 64 * s64
            tbl = synth.random_match_table(kmers, genome_length=2_000_000)[:, 0, 0]
            for row in (tbl, None):
                vectors = pc.lattice(kmers, nbins, bbits, row, adjust)
                names = [name for name, _ in vectors]
                assert len(set(names)) == len(names)
                for skip in (0, 1):
                    oracle.set_ext(adjust, skip)
                    how = dict(bbits=bbits, rtab_row=row, collision_adjust=bool(adjust), fit_skip=bool(skip))
                    for name, v in vectors:
                        ref = pc.exact_fit(v, kmers, nbins, **how)
                        jac, core64, acc64, failed64 = fp64_fit(v, kmers, nbins, bbits, row, adjust, skip)
                        got, failed = oracle.fit(jac, kmers, nbins)
                        where = (s64, bbits, nk, adjust, row is not None, skip, name, v)
                        assert failed == failed64 == ref.failed, where
                        assert got[0] == np.float32(core64) and got[1] == np.float32(acc64), where
                        assert within_one_ulp(got[0], ref.core) and within_one_ulp(got[1], ref.acc), (where, got, ref)
                        worst = max(worst, abs(core64 - float(ref.core_exact)), abs(acc64 - float(ref.acc_exact)))
                        # a J exactly on the floor (5 bins of nbins after the integer adjustment, no table entry subtracted) is usable in every arithmetic:
                        # both sides of the test are the same quotient
                        on_floor = [m for m in ref.floor_margins if m == 0]
                        assert not on_floor or row is None, where
                        smallest_margin = min(smallest_margin, min(abs(m) for m in ref.floor_margins if m != 0))
                        n_points += 1
    finally:
        oracle.set_ext(0, 0)
    print("lattice points %d, largest |oracle fp64 - exact| %.3g, smallest floor margin off the floor %.3g"
          % (n_points, worst, smallest_margin))
    assert worst <= pc.FP64_ERR
    # no lattice point sits closer to a decision than fp64 resolves by a wide margin (2^-53 is 1.1e-16)
    assert smallest_margin >= 1e-10


def test_the_lattice_holds_what_it_is_named_for():
    kmers = pc.kmers_of(5)
    tbl = synth.random_match_table(kmers)[:, 0, 0]
    for row in (None, tbl):
        fits = {name: {skip: pc.exact_fit(v, kmers, 1024, rtab_row=row, fit_skip=bool(skip)) for skip in (0, 1)}
                for name, v in pc.lattice(kmers, 1024, rtab_row=row)}
        if row is None:
            assert pc.smallest_usable(0, 1024) == 5
        assert (fits["all"][0].core, fits["all"][0].acc, fits["all"][0].failed) == (0, 0, False)
        assert all(max(fits["one-off-k%d" % k][0].core, fits["one-off-k%d" % k][0].acc) > 0 for k in range(5))
        assert fits["floor-1-k0"][0].failed and fits["floor-1-k0"][0].n_used == 0          # no usable point
        assert fits["floor-1-k1"][0].failed and fits["floor-1-k1"][0].n_used == 1          # one
        assert not fits["floor-1-k2"][0].failed and fits["floor-1-k2"][0].n_used == 2      # exactly two
        assert fits["floor-1-k4"][0].n_used == 4                                           # nk - 1
        for name in ("floor-1-k0", "floor-1-k1", "floor-1-k2"):                            # the rescued fits
            assert not fits[name][1].failed and fits[name][1].n_used == 4
        for i in (0, 1, 2, 4):
            assert fits["floor+0-k%d" % i][0].n_used == fits["floor+1-k%d" % i][0].n_used == 5
        assert fits["hole-k2"][0].n_used == 2 and fits["hole-k2"][1].n_used == 4
        assert fits["hole-k2"][0].core != fits["hole-k2"][1].core
        assert fits["rising"][0].slope > 0 and fits["rising"][0].core == 0 and fits["rising"][0].acc > 0
        assert fits["steep"][0].intercept > 0 and fits["steep"][0].acc == 0 and fits["steep"][0].core > 0
        if row is None:
            assert fits["constant"][0].slope == 0 and fits["constant"][0].core_exact == 0


# ---- the tripwire bands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s64,nk", pc.TRIPWIRE_SHAPES)
def test_every_tripwire_band_is_a_thousand_ulps_wide(s64, nk):
    kmers = pc.kmers_of(nk)
    nbins = 64 * s64
    row = synth.random_match_table(kmers)[:, 0, 0]
    v = pc.tripwire_vector(kmers, nbins)
    t = pc.tripwire(v, kmers, nbins, rtab_row=row)
    weights = pc.slope_weights(kmers)
    for slope in (0, 1, 2):
        print("s64 %d nk %d slope %d: d(v) %.6g, smallest single-count move %.3g = %.0f float32 ulps, sees k %s"
              % (s64, nk, slope, t[slope]["centre"], t[slope]["gap"], t[slope]["ulps"], t[slope]["visible"]))
        assert t[slope]["ulps"] >= 1000
        assert 0 < t[slope]["inner"][0] < t[slope]["outer"][0] or 0 < t[slope]["inner"][1] < t[slope]["outer"][1]
    # the core distance cannot see a k whose slope weight is 0 (the middle one of an odd, evenly spaced list)
    assert t[0]["visible"] == [k for k in range(nk) if weights[k] != 0]
    assert t[1]["visible"] == t[2]["visible"] == list(range(nk))
    # the boundaries separate d(v) from every move, in float32 as the device applies them
    centre, moves = pc.band(v, kmers, nbins, rtab_row=row)
    d = np.array([[centre.core, centre.acc]] + [[f.core, f.acc] for _, _, f in moves], dtype=np.float32)
    for slope in (0, 1, 2):
        inside_outer = oracle.assign_threshold(d, slope, *t[slope]["outer"]) <= 0
        inside_inner = oracle.assign_threshold(d, slope, *t[slope]["inner"]) <= 0
        assert inside_outer[0] and not inside_inner[0]
        for (k, _, _), out, inn in zip(moves, inside_outer[1:], inside_inner[1:]):
            if k in t[slope]["visible"]:
                assert out == inn, (slope, k)          # a moved pair is on the same side of both: one of them trips
            else:
                assert out and not inn


@pytest.mark.parametrize("s64,nk", pc.TRIPWIRE_SHAPES)
def test_bgmm_tripwire_models_on_the_cpu(s64, nk):
    from poppunk_amd.models import BGMMModel
    kmers = pc.kmers_of(nk)
    row = synth.random_match_table(kmers)[:, 0, 0]
    on, off, d0, dm = pc.bgmm_tripwire(pc.tripwire_vector(kmers, 64 * s64), kmers, 64 * s64, rtab_row=row)
    X = np.vstack([d0[None], dm])
    labels, resp = restated(X, on[0], on[1], on[2], on[3])
    margin = np.log(np.maximum(resp[:, 0], 1e-300)) - np.log(np.maximum(resp[:, 1], 1e-300))
    print("s64 %d nk %d: log responsibility ratio within / other %.3g at d(v), %.3g at most at a move"
          % (s64, nk, margin[0], margin[1:].max()))
    assert labels[0] == 0 and (labels[1:] == 1).all()
    assert margin[0] > 5 and margin[1:].max() < -5
    labels_off, _ = restated(X, off[0], off[1], off[2], off[3])
    assert labels_off[0] == 1
    for m in (on, off):
        assert BGMMModel(*m).model.n_jitter == 0
