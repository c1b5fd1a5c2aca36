"""The fit's answer for single counts: one planted pair per vector of plant_counts.lattice() -- every bin equal, one
mismatch at one k (the smallest non-zero distances), a count one below, on and one above the smallest usable count c*
at k index 0, 1, 2 and the last (a failed fit, one usable point, exactly two, nk - 1, and under "ext_fit_skip" the rescued
fits), a hole at k index 2 with high counts after it (where truncating and skipping differ), a rising vector (core
exactly 0), a steep fall (accessory exactly 0) and a constant one (the exact slope is 0) -- against
plant_counts.exact_fit, the fit in exact and 50-digit arithmetic.

Every implementation of the fit meets it: the tile epilogue (fit_packed / fit_general over PackW), the windowed register
(PackWide), the one-launch k-split path (the LDS table at s = 1 024, "from the parts" elsewhere: PackParts), the two-pass
counts + regress_packed_kernel path, the pair list (PackRows), the raw planes of 3 and 4 dwords at sketchsize64 156 and
the generic-bbits kernel with regress_counts_row, with the random-match table and without, under both settings of
"ext_fit_skip" and, where it is in effect, of "ext_collision_adjust" (kernel and oracle flipped together).

Checks, per target and route:
  * the row is a failed fit exactly where the reference says so: the pair alone through engine.dist_pairs reports
    n_failed 1 or 0 (an all-equal pair is (0, 0) and NOT failed), a failed row is (0, 0), and the job's n_failed is the
    CPU oracle's;
  * routes DESIGN.md promises the same bits give torch.equal rows;
  * |got - exact| <= 1 float32 ulp of the exact value + A.
A = plant_counts.FIT_ALLOWANCE = 16 x 1.8e-14 = 2.88e-13: 1.71e-14 is the largest |oracle fp64 - exact| measured over
these lattices before rounding (tests/test_plant_counts_host.py); the device's fast path multiplies nk table powers where
the oracle takes one exp, hence the factor.  Where the exact value is 0 (a clamped slope or intercept, the constant
vector's core) A alone bounds the result.  No lattice point is excluded for a small decision margin: the smallest
relative distance of a J from the floor is 1.4e-9 (a count of 5 at k = 29 with the table), seven orders above fp64's."""
import functools

import numpy as np
import pytest
import torch

import plant_counts as pc
from oracle import oracle
from poppunk_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

A = pc.FIT_ALLOWANCE          # 2.88e-13, from the measured 1.71e-14 (module docstring)
TILE = dict(ksplit=0, ksplit_long=0, rank_planes=0)
# the routes of the default shape: options, end of the kernel's name; all five give the same bits
ROUTES = [("tile epilogue", TILE, "<256x32,lds-dma>"),
          ("k-split", dict(), "k-split fused>"),
          ("wide", dict(TILE, wide_kpg=2), ",wide>"),
          ("two passes", dict(ksplit=100000, ksplit_fused=0), "regress_packed_kernel")]


def last_kernel():
    return _lib.lib().ppk_last_kernel_name().decode()


@functools.lru_cache(maxsize=None)
def population(s64, bbits, nk, adjust, table):
    kmers = pc.kmers_of(nk)
    nbins = 64 * s64
    tbl = synth.random_match_table(kmers) if table else None
    row = tbl[:, 0, 0] if table else None
    vectors = pc.lattice(kmers, nbins, bbits, row, bool(adjust))
    n = 300 if s64 == 16 else 100
    step = (7, 6) if n == 300 else (2, 2)
    pairs = [(n - 1 - step[1] * i, step[0] * i) for i in range(len(vectors))]          # all disjoint
    pairs = [(max(p), min(p)) for p in pairs]                                          # (higher, lower)
    assert len({s for p in pairs for s in p}) == 2 * len(pairs)
    sk = synth.make_sketches(n, kmers, sketchsize64=s64, bbits=bbits, cluster_size=10, seed=3)[0]
    bins = oracle.deslice(sk, s64, bbits).astype(np.uint16)
    pc.plant(bins, [(lo, hi, v) for (hi, lo), (_, v) in zip(pairs, vectors)], bbits=bbits, seed=4,
             first=(0, 63, nbins - 64, nbins - 1))
    return dict(sk=synth.bitslice(bins, bbits), kmers=kmers, tbl=tbl, row=row, vectors=vectors, pairs=pairs, n=n)


def references(pop, s64, bbits, adjust, skip):
    return [pc.exact_fit(v, pop["kmers"], 64 * s64, bbits=bbits, rtab_row=pop["row"], collision_adjust=bool(adjust),
                         fit_skip=bool(skip)) for _, v in pop["vectors"]]


def target_rows(pop, dist):
    n = pop["n"]
    rows = [lo * n - lo * (lo + 1) // 2 + (hi - lo - 1) for hi, lo in pop["pairs"]]
    return dist[torch.as_tensor(rows, device=dist.device)]


def check_rows(got, refs, pop, what):
    got = got.cpu().numpy()
    worst = 0.0
    for (name, v), g, ref in zip(pop["vectors"], got, refs):
        if ref.failed:
            assert g[0] == 0 and g[1] == 0, (what, name, v, g)
        for x, want, exact in ((g[0], ref.core, ref.core_exact), (g[1], ref.acc, ref.acc_exact)):
            err = abs(float(x) - float(want))
            assert err <= pc.ulp32(want) + A, (what, name, v, "got %r, exact %r (%s)" % (x, want, exact))
            worst = max(worst, err / pc.ulp32(want) if want != 0 else err / A)
    return worst


def run_route(ppk_option, pop, s64, bbits, options, kernel):
    for name, value in options.items():
        ppk_option(name, value)
    db = engine.SketchDB(pop["sk"], s64, bbits)
    try:
        dist, failed = engine.dist(db, None, pop["kmers"], pop["tbl"], random_correct=pop["tbl"] is not None)
        torch.cuda.synchronize()
        assert last_kernel().endswith(kernel), last_kernel()
        return target_rows(pop, dist).clone(), int(failed.item())
    finally:
        db.close()


def pair_list(pop, s64, bbits, refs, dense_rows):
    """engine.dist_pairs: the whole target list (the dense rows' bits), then every target alone for its failed flag"""
    db = engine.SketchDB(pop["sk"], s64, bbits)
    try:
        kw = dict(random_correct=pop["tbl"] is not None)
        ids = torch.as_tensor([[lo, hi] for hi, lo in pop["pairs"]], dtype=torch.int64, device="cuda:%d" % db.device)
        rows, failed = engine.dist_pairs(db, None, pop["kmers"], pop["tbl"], pairs=ids, **kw)
        assert torch.equal(rows, dense_rows) and int(failed.item()) == sum(r.failed for r in refs)
        for i, ((name, v), ref) in enumerate(zip(pop["vectors"], refs)):
            one, f = engine.dist_pairs(db, None, pop["kmers"], pop["tbl"], pairs=ids[i:i + 1], **kw)
            assert int(f.item()) == int(ref.failed), (name, v, "failed flag")
            assert torch.equal(one, dense_rows[i:i + 1]), (name, v)
        return rows
    finally:
        db.close()


def oracle_failed(pop, s64, bbits):
    return oracle.query(pop["sk"], None, pop["kmers"], s64, bbits, pop["tbl"], random_correct=pop["tbl"] is not None,
                        threads=8)[1]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("table", [True, False])
def test_default_shape_through_every_route(ppk_option, table, skip):
    s64, bbits, nk, adjust = 16, 14, 5, 0
    pop = population(s64, bbits, nk, adjust, table)
    refs = references(pop, s64, bbits, adjust, skip)
    ppk_option("ext_fit_skip", skip)
    oracle.set_ext(adjust, skip)
    try:
        want_failed = oracle_failed(pop, s64, bbits)
    finally:
        oracle.set_ext(0, 0)
    assert want_failed >= sum(r.failed for r in refs) and (skip or any(r.failed for r in refs))
    first = None
    for name, options, kernel in ROUTES:
        rows, failed = run_route(ppk_option, pop, s64, bbits, options, kernel)
        assert failed == want_failed, (name, failed, want_failed)
        worst = check_rows(rows, refs, pop, name)
        if first is None:
            first = rows
            print("table %d skip %d: n_failed %d, worst |got - exact| %.3g float32 ulps (or of A at an exact 0)"
                  % (table, skip, failed, worst))
        assert torch.equal(rows, first), name          # the same statements on the same counts: the same bits
        reset(ppk_option, options)
    pair_list(pop, s64, bbits, refs, first)


def reset(ppk_option, options):
    """the routes' options back at the library's defaults (the fixture restores what the test found at its end)"""
    defaults = dict(ksplit=1200, ksplit_long=1, rank_planes=1, wide_kpg=0, ksplit_fused=1)
    for name in options:
        ppk_option(name, defaults[name])


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("table", [True, False])
@pytest.mark.parametrize("s64,bbits,nk,adjust", pc.LATTICE_SHAPES[1:])
def test_other_shapes_through_their_default_route(ppk_option, s64, bbits, nk, adjust, table, skip):
    """(156, 14) with 6 and 9 k -- count registers of 3 and 4 dwords, a long sketch: the k-split path fitted from the
    parts -- and (20, 10) with 4 k, the generic-bbits kernel, where 1 280 >> 10 = 1 puts the collision adjustment in
    effect"""
    pop = population(s64, bbits, nk, adjust, table)
    refs = references(pop, s64, bbits, adjust, skip)
    ppk_option("ext_fit_skip", skip)
    ppk_option("ext_collision_adjust", adjust)
    oracle.set_ext(adjust, skip)
    try:
        want_failed = oracle_failed(pop, s64, bbits)
    finally:
        oracle.set_ext(0, 0)
    rows, failed = run_route(ppk_option, pop, s64, bbits, {}, "generic>" if bbits != 14 else "fit from parts>")
    assert failed == want_failed
    worst = check_rows(rows, refs, pop, (s64, bbits, nk, adjust, table, skip))
    print("(%d, %d) %d k adjust %d table %d skip %d: n_failed %d, worst %.3g float32 ulps (or of A at an exact 0)"
          % (s64, bbits, nk, adjust, table, skip, failed, worst))
    if bbits == 14:          # the tile kernel's own epilogue on the raw planes of 3 and 4 dwords: the same bits
        tile, tile_failed = run_route(ppk_option, pop, s64, bbits, dict(ksplit=0, ksplit_long=0), "<256x32,lds-dma>")
        assert torch.equal(tile, rows) and tile_failed == failed
        reset(ppk_option, dict(ksplit=0, ksplit_long=0))
    pair_list(pop, s64, bbits, refs, rows)
