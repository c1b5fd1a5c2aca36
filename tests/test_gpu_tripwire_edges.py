"""Tripwire pairs for the fused edge lists (MODE_MASK, the line boundary, and MODE_BGMM) of every route of kernel 1.

"The edge list equals the list of another route" at a boundary from a quantile lets a count that is off by one through:
it rarely moves a pair across the boundary (profiles/NOTES_r10.md section 7: two hand mutations of the `fold2` epilogue
passed both fused cases).  Here 12 to 14 disjoint pairs of a population are planted (tests/plant_counts.py) so that all
of them match in exactly one common count vector v, and the boundaries are threaded, on the CPU and from the exact
reference, half a band either side of d(v): under the OUTER boundary every target is an edge, under the INNER one none
is, and one count more or less at any k the boundary kind can see moves a target across one of the two by a thousand
float32 ulps or more (asserted on the CPU in tests/test_plant_counts_host.py, with the measured widths).
  slope 0 (core distance)  cannot see the k whose slope weight is 0 (the middle one of an odd, evenly spaced list) --
                           asserted from the exact reference, not skipped;
  slope 1 (accessory) and slope 2 (a line chosen so that its normal has a component along every single-count move)
                           see every k;
  BGMM                     a two-component model whose within component is narrow around d(v) (every d(v +- e_k) goes
                           to the other component: checked with the numpy restatement, tests/test_plant_counts_host.py),
                           and the same model moved by one band, under which no target is an edge.

The targets sit at the position classes of tests/test_gpu_rank_fold2.py (pairs are (higher, lower) sample; the higher one
is the ref of a 256 x 32 tile):
  (181, 20)             both in one tile                (262, 45)   the higher sample on the strip (n = 300)
  (295, 273)            both on the strip               (252, 141)  a half tile
  (104, 9), (105, 13)   refs 2l and 2l + 1 of one lane  (62, 15), (190, 17)  refs 128 apart
  (120, 32), (121, 63)  first and last query row of a tile
  (75, 70)              q - r < 32 on the diagonal tile (n - 1, 0)  the corner
and, in the populations of 1 100 and 2 100, two pairs in later ref tiles.

Populations: at sketchsize64 16 the tripled related population of test_gpu_rank_fold2.planted(300) with its own events
(one pair at the cap of 63), planted under keep_coded so that the two-holder pair is still built; some of the targets'
matches are themselves two-holder values, so their vector is only right if the `fold2` epilogue adds its corrections --
the two mutations of NOTES_r10.  n = 1 100 and 2 100 are test_gpu_rank_shapes.py's plantings for 10 and 12 planes with
the targets on top (the threshold positions are left alone).  At sketchsize64 156 a tripled population of 100.

Every call is held to three checks: target membership as predicted; n_failed equal to the CPU oracle's; the whole list
equal to the two-step list (edge_threshold_dev / bgmm_edges_dev) of the same route's engine.dist output."""
import functools

import numpy as np
import pytest
import torch

import plant_counts as pc
from oracle import oracle
from poppunk_amd import _lib, engine, synth
from poppunk_amd.models import BGMMModel
from rank_fold2_model import MAX_PER_PAIR, SLOTS, block_counts, events_of, per_pair_max
from rank_model import unslice

pytestmark = pytest.mark.gpu

RAW = "dist_kernel_v2<256x32,lds-dma>"
TILE = dict(ksplit=0, ksplit_long=0)          # whole tiles, the tile kernel's own epilogue
# route: (sketchsize64, nk, n, options set before the database is created, end of the kernel's name, jobs)
ALL_JOBS = ("whole", "band", "itself", "host")
ROUTES = {
    "raw W=2": (16, 5, 300, dict(TILE, rank_planes=0), RAW, ALL_JOBS),
    "raw W=3": (156, 6, 300, dict(TILE), RAW, ("whole", "band")),
    "raw W=4": (156, 9, 300, dict(TILE), RAW, ("whole", "band")),
    "wide": (16, 5, 300, dict(TILE, rank_planes=0, wide_kpg=2), ",wide>", ("whole", "band")),
    "k-split fused": (16, 5, 300, dict(), "k-split fused>", ("whole", "band", "itself")),
    "fit from parts": (156, 6, 300, dict(), "fit from parts>", ("whole", "band", "itself")),
    "fit from parts, windowed": (16, 5, 300, dict(wide_kpg=2), "fit from parts>", ("whole",)),
    "rank 8": (16, 5, 300, dict(TILE, rank_planes=1, rank_fold=0, rank_fold2=0), ",rank 8>", ("whole", "band")),
    "rank 10": (16, 5, 1100, dict(TILE, rank_planes=1, rank_fold=0, rank_fold2=0), ",rank 10>", ("whole",)),
    "rank 12": (16, 5, 2100, dict(TILE, rank_planes=1, rank_fold=0, rank_fold2=0), ",rank 12>", ("whole",)),
    "fold": (16, 5, 300, dict(TILE, rank_planes=1, rank_fold=2, rank_fold2=0), ",rank 8,fold>", ("whole", "band")),
    "fold2": (16, 5, 300, dict(TILE, rank_planes=1, rank_fold=2, rank_fold2=2), ",rank 8,fold2>", ("whole", "band", "host")),
}
EVENTS = [1, 0, 3, 1, 2, 1, 1, 0, 1, 1, 2, 1, 0, 0]          # matches per k of each target that are two-holder values


def pairs_of(n):
    t = [(181, 20), (262, 45), (295, 273), (252, 141), (104, 9), (105, 13), (62, 15), (190, 17), (120, 32), (121, 63),
         (75, 70), (n - 1, 0)]
    if n > 300:
        t += [(n - 41, n - 300), (600, 291)]
    return t


def last_kernel():
    return _lib.lib().ppk_last_kernel_name().decode()


@functools.lru_cache(maxsize=None)
def population(s64, nk, n):
    """everything a case needs that no option changes: the planted sketches, the targets, the k list and table, the
    boundaries and models from the exact reference, the oracle's failed fits (self job and the handle against itself)"""
    kmers = pc.kmers_of(nk)
    nbins = 64 * s64
    tbl = synth.random_match_table(kmers)
    v = pc.tripwire_vector(kmers, nbins)
    pairs = pairs_of(n)
    # and one pair that is no tripwire: 3 equal bins at k index 1 leave its fit one usable point -- a failed fit, a
    # (0, 0) row inside every boundary, so that n_failed is not 0 in any job
    fails = tuple(3 if k == 1 else c for k, c in enumerate(v))
    assert pc.exact_fit(fails, kmers, nbins, rtab_row=tbl[:, 0, 0]).failed
    targets = [(lo, hi, v) for hi, lo in pairs] + [(55, 230, fails)]
    if (s64, n) == (16, 300):
        from test_gpu_rank_fold2 import planted
        bins = planted(300)[1].copy()
        pc.plant(bins, targets, events=EVENTS[:len(pairs)] + [0], seed=11, keep_coded=True)
        ev = events_of(bins)
        assert per_pair_max(ev) == MAX_PER_PAIR and block_counts(bins)[3] <= SLOTS          # the two-holder pair is built
        for (hi, lo), e in zip(pairs, EVENTS):
            assert int(((ev[:, 0] == hi) & (ev[:, 1] == lo)).sum()) == e * nk
    elif s64 == 16:
        from test_gpu_rank_shapes import Planter, plant_d10, plant_d12
        p = Planter(16, 5, n)
        {1100: plant_d10, 2100: plant_d12}[n](p)
        avoid = np.zeros((nk, nbins), dtype=bool)
        for k, blk, bit in (c[:3] for c in p.claims):
            avoid[k, blk * 64 + bit] = True
        bins = unslice(p.sk)
        at_thresholds = bins[:, avoid].copy()
        pc.plant(bins, targets, seed=11, avoid=avoid)
        assert np.array_equal(bins[:, avoid], at_thresholds)
    else:
        base = unslice(synth.make_sketches(n // 3, kmers, sketchsize64=s64, cluster_size=10)[0])
        bins = np.tile(base, (3, 1, 1))
        pc.plant(bins, targets, seed=11)
    sk = synth.bitslice(bins, 14)
    row = tbl[:, 0, 0]
    trip = pc.tripwire(v, kmers, nbins, rtab_row=row)
    weights = pc.slope_weights(kmers)
    assert trip[0]["visible"] == [k for k in range(nk) if weights[k] != 0]       # the core distance is blind to that k
    assert trip[1]["visible"] == trip[2]["visible"] == list(range(nk))
    on, off, _, _ = pc.bgmm_tripwire(v, kmers, nbins, rtab_row=row)
    failed = oracle.query(sk, None, kmers, s64, 14, tbl, threads=8)[1]
    failed_rect = oracle.query(sk, sk, kmers, s64, 14, tbl, threads=8)[1] if n == 300 else None
    assert failed >= 1          # (more where the rewritten sample now shares as little with others)
    return dict(sk=sk, kmers=kmers, tbl=tbl, pairs=pairs, trip=trip, models=(BGMMModel(*on), BGMMModel(*off)),
                failed=failed, failed_rect=failed_rect, fit=pc.exact_fit(v, kmers, nbins, rtab_row=row))


def calls(pop):
    """(name, fused call, two-step call on a distance tensor, are the targets edges) for the eight boundaries"""
    out = []
    for slope in (0, 1, 2):
        for which, inside in (("outer", True), ("inner", False)):
            x_max, y_max = pop["trip"][slope][which]
            out.append(("slope %d %s" % (slope, which),
                        dict(slope=slope, x_max=x_max, y_max=y_max), None, inside))
    for m, inside in zip(pop["models"], (True, False)):
        out.append(("bgmm %s" % ("on d(v)" if inside else "one band off"), None, m.model, inside))
    return out


def check(edges, failed, want_edges, want_failed, targets, inside, what):
    edges = edges.cpu().numpy() if torch.is_tensor(edges) else edges
    code = lambda e: e[:, 0] * (1 << 32) + e[:, 1]
    listed = np.isin(code(np.asarray(targets, dtype=np.int64)), code(edges.reshape(-1, 2)))
    hit = [t for t, there in zip(targets, listed) if there]
    assert hit == (targets if inside else []), (what, "targets listed", hit)
    assert int(failed) == want_failed, (what, "n_failed")
    assert np.array_equal(edges, want_edges.cpu().numpy()), (what, "not the two-step list")


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_targets_cross_the_boundary_with_one_count(ppk_option, route):
    s64, nk, n, options, kernel, jobs = ROUTES[route]
    pop = population(s64, nk, n)
    kmers, tbl = pop["kmers"], pop["tbl"]
    for name, value in options.items():
        ppk_option(name, value)
    db = engine.SketchDB(pop["sk"], s64, 14)
    try:
        if route == "fold2":
            assert db.fold2_planes == 8
        self_targets = [(lo, hi) for hi, lo in pop["pairs"]]
        rect_targets = [(a, n + b) for hi, lo in pop["pairs"] for a, b in ((hi, lo), (lo, hi))]
        dist, dist_failed = engine.dist(db, None, kmers, tbl)
        torch.cuda.synchronize()
        assert last_kernel().endswith(kernel), last_kernel()
        assert int(dist_failed.item()) == pop["failed"]
        rows = np.asarray([lo * n - lo * (lo + 1) // 2 + (hi - lo - 1) for hi, lo in pop["pairs"]])
        got = dist[torch.as_tensor(rows, device=dist.device)].cpu().numpy()
        print("%s: targets' distances off d(v) by at most %.3g (core), %.3g (accessory)"
              % (route, np.abs(got[:, 0] - pop["fit"].core).max(), np.abs(got[:, 1] - pop["fit"].acc).max()))
        bands = ((0, 37), (37, n - 40), (n - 40, n))          # cuts inside 32-row query tiles
        for what, line, model, inside in calls(pop):
            if line is not None:
                fused = lambda a, b=None, **kw: engine.dist_edges(a, b, kmers, tbl, **line, **kw)
                two_step = lambda d, n_ref=0: engine.edge_threshold_dev(d, line["slope"], line["x_max"], line["y_max"], n_ref=n_ref)
                host = lambda: engine.edges_host(db, None, kmers, tbl, **line)
            else:
                fused = lambda a, b=None, **kw: engine.dist_bgmm_edges(a, b, kmers, tbl, model=model, **kw)
                two_step = lambda d, n_ref=0: engine.bgmm_edges_dev(d, model, n_ref=n_ref)
                host = lambda: engine.bgmm_edges_host(db, None, kmers, tbl, model=model)
            want = two_step(dist)
            if "whole" in jobs:
                e, f = fused(db)
                torch.cuda.synchronize()
                assert last_kernel().endswith(kernel), (what, last_kernel())
                check(e, f.item(), want, pop["failed"], self_targets, inside, (route, what, "whole"))
            if "band" in jobs:
                parts = [fused(db, q_begin=a, q_end=b) for a, b in bands]
                check(torch.cat([p[0] for p in parts]), sum(int(p[1].item()) for p in parts), want, pop["failed"],
                      self_targets, inside, (route, what, "bands"))
            if "itself" in jobs:
                rect, rect_failed = engine.dist(db, db, kmers, tbl)
                e, f = fused(db, db)
                assert int(rect_failed.item()) == pop["failed_rect"]
                check(e, f.item(), two_step(rect, n), pop["failed_rect"], rect_targets, inside, (route, what, "itself"))
            if "host" in jobs:
                e, f = host()
                check(e, f, want, pop["failed"], self_targets, inside, (route, what, "host"))
    finally:
        db.close()
