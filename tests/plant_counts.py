"""Sketches planted so that chosen pairs have chosen match-count vectors, and the exact answer those vectors fit to --
shared by tests/test_plant_counts_host.py, test_gpu_tripwire_edges.py and test_gpu_fit_lattice.py.

plant()      rewrites the bins of chosen disjoint pairs so that pair (q, r) matches in exactly vector[k] bins at every k,
             at positions drawn over all blocks, some of the matches as values that q and r alone hold (the events of
             the two-holder coded copies), and recounts every target with oracle.match_counts.
exact_fit()  step a6 of oracle/ppk_oracle.c (with a4 and a5 in front of it) without fp64: J_k and the floor test
             J < 5/nbins are fractions.Fraction (a float32 table entry is an exact rational), the regression is
             sum_k a_k log J_k with rational weights, logarithm and 1 - exp at 50 digits (mpmath), the result rounded
             to float32 once.  A slope or intercept that is 0 in exact arithmetic (every usable J equal; every J 1) is
             found as such, not as a residue of rounding.
band()       the exact distances of v and of every v +- e_k: what a tripwire boundary is threaded between.
"""
import collections
from fractions import Fraction

import mpmath
import numpy as np

from oracle import oracle
from poppunk_amd import synth

DPS = 50

# The largest |oracle fp64 - exact| of core and accessory distances before rounding, over every lattice of
# LATTICE_SHAPES with and without the random-match table and under both settings of the fit's [EXT] switches
# (tests/test_plant_counts_host.py measures it and fails if it grows past this figure): 1.71e-14 measured, at a fit
# through two points two k apart at sketchsize64 156 (the intercept is the difference of two logarithms times 14);
# a fit through every k stays below 2e-15.
FP64_ERR = 1.8e-14
# Allowance A of tests/test_gpu_fit_lattice.py: the device's fast path multiplies nk table powers where the oracle takes
# one exp, so 16 times the oracle's own fp64 error: 2.88e-13, a 3 000th of a float32 ulp at a core distance of 0.01.
FIT_ALLOWANCE = 16 * FP64_ERR

LATTICE_SHAPES = [(16, 14, 5, 0), (156, 14, 6, 0), (156, 14, 9, 0), (20, 10, 4, 0), (20, 10, 4, 1)]      # s64, bbits, nk, [EXT] a4
TRIPWIRE_SHAPES = [(16, 5), (156, 6), (156, 9)]          # s64, nk: count registers of 2, 3 and 4 dwords


def kmers_of(nk):
    """nk k-mer lengths from 13 to 29 (the default list at nk = 5)"""
    return np.round(np.linspace(13, 29, nk)).astype(np.int32)

Fit = collections.namedtuple("Fit", "core acc failed n_used floor_margins slope intercept core_exact acc_exact")


# ---- planting --------------------------------------------------------------------------------------------------------
def _fresh(bins, k, pos, rng, bbits):
    """one value per position that no sample holds there"""
    vals = rng.integers(0, 1 << bbits, size=len(pos)).astype(bins.dtype)
    for _ in range(200):
        clash = (bins[:, k, pos] == vals[None, :]).any(axis=0)
        if not clash.any():
            return vals
        vals[clash] = rng.integers(0, 1 << bbits, size=int(clash.sum())).astype(bins.dtype)
    raise ValueError("no free bin value at some position of k index %d" % k)


def _draw(ok, count, first, rng, what):
    """`count` of the positions where `ok`: those of `first` before the others, the others in a drawn order"""
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    cand = np.nonzero(ok)[0]
    if len(cand) < count:
        raise ValueError("%s: %d positions needed, %d may be rewritten" % (what, count, len(cand)))
    lead = np.asarray([p for p in first if ok[p]], dtype=np.int64)
    rest = rng.permutation(np.setdiff1d(cand, lead))
    return np.concatenate([lead, rest])[:count]


def recount(bins, targets, bbits=14):
    """[targets, nk] match counts of the target pairs, by oracle.match_counts from the bit-sliced sketches"""
    s64 = bins.shape[2] // 64
    qs = synth.bitslice(bins[[t[0] for t in targets]], bbits)
    rs = synth.bitslice(bins[[t[1] for t in targets]], bbits)
    c = oracle.match_counts(rs, qs, s64, bbits).reshape(len(targets), len(targets), bins.shape[1])     # row = q * n_ref + r
    return c[np.arange(len(targets)), np.arange(len(targets))]


def plant(bins, targets, bbits=14, events=0, seed=1, first=(), avoid=None, keep_coded=False):
    """bins [n, nk, nbins] uint16, rewritten in place; targets: (q, r, vector) over pairwise disjoint samples.  Pair
    (q, r) ends with exactly vector[k] equal bins at every k: natural matches too many are taken away (r gets a value no
    sample holds there), matches missing are added (r takes q's value), and `events` (a number, or one per target) of
    the matches at every k are values q and r alone hold (both get the same unheld value).  Positions are drawn from
    all blocks by a generator seeded with `seed`; positions listed in `first` are used before the drawn ones wherever
    they qualify.  avoid: bool [nk, nbins], positions never touched.  keep_coded: no sample is taken out of a value with
    exactly three holders and no value with one holder gains a second (either would make an event of some pair), so
    the events of the population stay what they were, plus the planted ones.
    Returns one list per target of the rewritten positions per k; raises where a recount is off."""
    n, nk, nbins = bins.shape
    samples = [s for q, r, _ in targets for s in (q, r)]
    if len(set(samples)) != len(samples) or min(samples) < 0 or max(samples) >= n:
        raise ValueError("target samples must be distinct samples of the population")
    per_target = [events] * len(targets) if np.isscalar(events) else list(events)
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.ones((nk, nbins), dtype=bool) if avoid is None else ~np.asarray(avoid, dtype=bool)
    touched = []
    for (q, r, vec), n_ev in zip(targets, per_target):
        if len(vec) != nk or min(vec) < n_ev or max(vec) > nbins:
            raise ValueError("vector %r does not fit nk = %d, nbins = %d, %d events" % (tuple(vec), nk, nbins, n_ev))
        rows = []
        for k in range(nk):
            what = "pair (%d, %d) k index %d" % (q, r, k)
            match = bins[q, k] == bins[r, k]
            hq = (bins[:, k, :] == bins[q, k][None, :]).sum(axis=0)
            hr = (bins[:, k, :] == bins[r, k][None, :]).sum(axis=0)
            r_ok = free[k] & ((hr != 3) if keep_coded else True)
            ev = _draw(~match & r_ok & ((hq != 3) if keep_coded else True), n_ev, first, rng, what + " events")
            taken = np.zeros(nbins, dtype=bool)
            taken[ev] = True
            need = int(vec[k]) - n_ev - int(match.sum())
            if need < 0:
                pos = _draw(match & r_ok, -need, first, rng, what + " matches to remove")
                bins[r, k, pos] = _fresh(bins, k, pos, rng, bbits)
            else:
                pos = _draw(~match & ~taken & r_ok & ((hq != 1) if keep_coded else True), need, first, rng,
                            what + " matches to add")
                bins[r, k, pos] = bins[q, k, pos]
            if n_ev:
                bins[q, k, ev] = bins[r, k, ev] = _fresh(bins, k, ev, rng, bbits)
            rows.append(np.sort(np.concatenate([ev, pos])))
        touched.append(rows)
    got = recount(bins, targets, bbits)
    want = np.asarray([t[2] for t in targets], dtype=np.int64)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("planted counts are off for targets %s: %s instead of %s" % (bad, got[bad], want[bad]))
    return touched


# ---- the exact answer ------------------------------------------------------------------------------------------------
def jaccard(count, nbins, bbits=14, jr=None, collision_adjust=False):
    """a4 and a5 as exact rationals: the (integer) collision adjustment, count / nbins, the random-match correction
    with the float32 table entry `jr` as the rational it is"""
    expected = nbins >> bbits
    inter = int(count)
    if collision_adjust and expected:
        inter = max(inter - expected, 0) * nbins // (nbins - expected)
    obs = Fraction(inter, nbins)
    if jr is None:
        return obs
    jr = Fraction(float(jr))
    return max(obs - jr, Fraction(0)) / (1 - jr)


def smallest_usable(k_index, nbins, bbits=14, rtab_row=None, collision_adjust=False):
    """c*: the smallest count whose J passes the floor test at this k"""
    jr = None if rtab_row is None else rtab_row[k_index]
    return next(c for c in range(nbins + 1) if jaccard(c, nbins, bbits, jr, collision_adjust) >= Fraction(5, nbins))


def _round32(x):
    """an mpf rounded to float32 once (to nearest even, straight from 50 digits)"""
    with mpmath.workprec(24):
        return np.float32(float(+x))


def _log_sum(weights, js):
    """sum_i w_i log J_i with rational w_i: equal J are taken together and J = 1 dropped first, so a sum that is 0 in
    exact arithmetic comes out as the integer 0"""
    by_j = collections.defaultdict(Fraction)
    for w, j in zip(weights, js):
        if j != 1:
            by_j[j] += w
    terms = [(w, j) for j, w in by_j.items() if w != 0]
    if not terms:
        return 0
    total = mpmath.fsum((mpmath.mpf(w.numerator) / w.denominator) * mpmath.log(mpmath.mpf(j.numerator) / j.denominator)
                        for w, j in terms)
    assert abs(total) > mpmath.mpf(10) ** -35, "a sum of logarithms too close to 0 to sign at 50 digits"
    return total


def exact_fit(vector, kmers, nbins, bbits=14, rtab_row=None, collision_adjust=False, fit_skip=False):
    """Fit(core, acc, failed, n_used, floor_margins, slope, intercept, core_exact, acc_exact): core and acc float32,
    floor_margins (J_k - floor) / floor per k (negative: unusable), slope and intercept as floats (their distance from
    0 is the margin of the two clamps), core_exact / acc_exact the 50-digit values before rounding"""
    with mpmath.workdps(DPS):
        floor = Fraction(5, nbins)
        js = [jaccard(c, nbins, bbits, None if rtab_row is None else rtab_row[i], collision_adjust)
              for i, c in enumerate(vector)]
        margins = [float((j - floor) / floor) for j in js]
        used = []
        for i, j in enumerate(js):
            if j < floor:
                if fit_skip:
                    continue
                break
            used.append(i)
        zero = mpmath.mpf(0)
        if len(used) < 2:
            return Fit(np.float32(0), np.float32(0), True, len(used), margins, 0.0, 0.0, zero, zero)
        xs = [Fraction(int(kmers[i])) for i in used]
        nn, sx, sxx = len(xs), sum(xs), sum(x * x for x in xs)
        a = [(nn * x - sx) / (nn * sxx - sx * sx) for x in xs]          # slope = sum a_i y_i
        b = [(1 - ai * sx) / nn for ai in a]                            # intercept = (sy - slope sx) / n = sum b_i y_i
        uj = [js[i] for i in used]
        slope, icpt = _log_sum(a, uj), _log_sum(b, uj)
        core = -mpmath.expm1(slope) if slope < 0 else zero
        acc = -mpmath.expm1(icpt) if icpt < 0 else zero
        return Fit(_round32(core), _round32(acc), False, nn, margins, float(slope), float(icpt), core, acc)


def slope_weights(kmers):
    """a_k of the slope when every k is usable (a k with a_k = 0 is invisible to the core distance)"""
    xs = [Fraction(int(k)) for k in kmers]
    nn, sx, sxx = len(xs), sum(xs), sum(x * x for x in xs)
    return [(nn * x - sx) / (nn * sxx - sx * sx) for x in xs]


def band(vector, kmers, nbins, **how):
    """(fit of v, [(k index, +1 | -1, fit of v + sign e_k)]) for every single-count move that stays within 0 .. nbins"""
    moves = []
    for k in range(len(vector)):
        for sign in (1, -1):
            if 0 <= vector[k] + sign <= nbins:
                v = list(vector)
                v[k] += sign
                moves.append((k, sign, exact_fit(v, kmers, nbins, **how)))
    return exact_fit(vector, kmers, nbins, **how), moves


def ulp32(x):
    """one float32 unit in the last place at |x| (0 at 0: a reference of exactly 0 allows no float32 error)"""
    x = np.float32(abs(x))
    return float(np.spacing(x)) if x != 0 else 0.0


# ---- the vectors the tests plant -------------------------------------------------------------------------------------
DEFAULT_KMERS = (13, 17, 21, 25, 29)
FALLING = (456, 419, 368, 334, 268)          # nbins 1024, k 13 .. 29: a related pair, every k well above the floor
STEEP = (1024, 377, 139, 51, 19)             # log J falls so fast that the intercept is positive: accessory exactly 0


def falling(kmers, nbins):
    """a falling mid-range vector: FALLING at the default shape, the same curve (1 - a)(1 - c)^k elsewhere"""
    if nbins == 1024 and tuple(int(k) for k in kmers) == DEFAULT_KMERS:
        return FALLING
    return tuple(int(round(nbins * 0.685 * 0.9674 ** int(k))) for k in kmers)


def tripwire_vector(kmers, nbins):
    """the common vector of the tripwire pairs: FALLING at the default shape; at the longer sketches a steeper curve
    (a = 0.3, c = 0.12) -- a single count moves the accessory distance by about |b_k| (1 - c)^-k / nbins, and at 9 984
    bins the curve of FALLING leaves that under 1 000 float32 ulps at the k where the intercept weight b_k is small"""
    if nbins == 1024 and tuple(int(k) for k in kmers) == DEFAULT_KMERS:
        return FALLING
    return tuple(int(round(nbins * 0.7 * 0.88 ** int(k))) for k in kmers)


def lattice(kmers, nbins, bbits=14, rtab_row=None, collision_adjust=False):
    """[(name, vector)]: the count vectors that sit on every decision of the fit -- all bins equal; one mismatch at one
    k; c* - 1, c*, c* + 1 (c* the smallest usable count of that k, from the exact floor test) at k index 0, 1, 2 and
    the last on a falling vector; a count below the floor at k index 2 with high counts after it; a rising vector; a
    steep fall; a constant vector"""
    nk = len(kmers)
    mid = falling(kmers, nbins)
    out = [("all", (nbins,) * nk)]
    for k in range(nk):
        out.append(("one-off-k%d" % k, tuple(nbins - (i == k) for i in range(nk))))
    for i in sorted({0, 1, 2, nk - 1}):
        c = smallest_usable(i, nbins, bbits, rtab_row, collision_adjust)
        for d in (-1, 0, 1):
            out.append(("floor%+d-k%d" % (d, i), tuple(c + d if j == i else mid[j] for j in range(nk))))
    high = [int(round(nbins * f)) for f in np.linspace(0.88, 0.6, nk)]
    high[2] = 1
    out.append(("hole-k2", tuple(high)))
    out.append(("rising", tuple(reversed(mid))))
    if nbins == 1024 and nk == 5:
        out.append(("steep", STEEP))
    else:
        out.append(("steep", tuple(int(round(nbins * (19.0 / 1024) ** (i / (nk - 1.0)))) for i in range(nk))))
    out.append(("constant", (int(round(0.3 * nbins)),) * nk))
    return out


# ---- tripwire boundaries ---------------------------------------------------------------------------------------------
SLOPE2_RATIOS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0)      # x_max / y_max candidates of the slope-2 line


def tripwire(vector, kmers, nbins, **how):
    """For each boundary kind of line_dist (0: core, 1: accessory, 2: a line with both intercepts) an outer and an inner
    boundary half a band either side of d(v), from the exact reference: {slope: dict(outer=(x_max, y_max), inner=...,
    visible=[k ...], gap=..., ulps=...)}.  `gap` is the smallest change a single-count move at a visible k makes to what
    the kind measures (core; accessory; core + ratio * accessory), `ulps` that gap in float32 units in the last place
    of the measured value.  A k is invisible to a kind when neither move at it changes the measured value at all (the
    k whose slope weight is 0, for the core distance).  Under the outer boundary d(v) is inside and every d(v +- e_k)
    that moves outwards is outside; under the inner one d(v) is outside and every inward move inside."""
    centre, moves = band(vector, kmers, nbins, **how)
    assert not centre.failed and centre.core_exact > 0 and centre.acc_exact > 0
    nk = len(vector)

    def kind(measure, boundary):
        h0 = measure(centre)
        delta = {(k, s): measure(f) - h0 for k, s, f in moves}
        visible = [k for k in range(nk) if all(delta[(k, s)] != 0 for s in (1, -1) if (k, s) in delta)]
        gap = min(abs(delta[(k, s)]) for k, s in delta if k in visible)
        return dict(outer=boundary(float(h0 + gap / 2)), inner=boundary(float(h0 - gap / 2)), visible=visible,
                    gap=float(gap), ulps=float(gap) / ulp32(float(h0)), centre=float(h0))

    out = {0: kind(lambda f: f.core_exact, lambda b: (b, 1.0)), 1: kind(lambda f: f.acc_exact, lambda b: (1.0, b))}
    best = None
    for ratio in SLOPE2_RATIOS:      # edge iff core * y_max + acc * x_max <= x_max * y_max, i.e. core + ratio * acc <= x_max
        t = kind(lambda f, ratio=ratio: f.core_exact + ratio * f.acc_exact, lambda b, ratio=ratio: (b, b / ratio))
        t["ratio"] = ratio
        if len(t["visible"]) == nk and (best is None or t["ulps"] > best["ulps"]):
            best = t
    assert best is not None, "no slope-2 line sees every k"
    out[2] = best
    return out


def bgmm_tripwire(vector, kmers, nbins, **how):
    """Two two-component models (weights, means, covariances, scale, within label, between label) for
    models.BGMMModel: the within component (label 0) of the first is narrow around d(v) -- d(v) is assigned to it and
    every d(v +- e_k) to the broad other one; the second is the first with its narrow component moved by one band, onto
    the nearest d(v +- e_k), which sends d(v) to the other component.  The narrow component's deviations are a fixed
    fraction of the smallest accessory move (every single-count move changes the accessory distance), the fraction
    chosen so that the switch between the components lies half-way to that move.  Also returns d(v) and the moves'
    distances as float64 [.., 2] arrays for the CPU check."""
    centre, moves = band(vector, kmers, nbins, **how)
    d0 = np.array([float(centre.core_exact), float(centre.acc_exact)])
    dm = np.array([[float(f.core_exact), float(f.acc_exact)] for _, _, f in moves])
    gy = float(np.abs(dm[:, 1] - d0[1]).min())
    assert gy > 0
    broad = 0.3
    # Equal weights, and the broad density is flat over the band, so at z deviations along y the narrow component leads
    # by log(broad^2 / (sigma_x sigma_y)) - z^2 / 2.  A move may leave the core distance where it is, so the decision is
    # taken along y alone: sigma_x = 100 sigma_y keeps every move's x offset well inside the narrow component.  The
    # switch z0 is to lie half-way to the smallest move: sigma_y = gy / (2 z0), z0^2 = 2 log(broad^2 / (100 sigma_y^2)).
    sigma = gy / 8.0
    for _ in range(60):
        z0 = np.sqrt(2.0 * np.log(broad * broad / (100.0 * sigma * sigma)))
        sigma = gy / (2.0 * z0)
    cov = np.array([np.diag([1e4 * sigma * sigma, sigma * sigma]), np.diag([broad * broad, broad * broad])])
    weights = np.array([0.5, 0.5])
    scale = np.array([1.0, 1.0])
    means = np.array([d0, [0.3, 0.5]])
    nearest = dm[np.argmin(np.abs(dm[:, 1] - d0[1]))]
    shifted = np.array([nearest, [0.3, 0.5]])
    return (weights, means, cov, scale, 0, 1), (weights, shifted, cov, scale, 0, 1), d0, dm
