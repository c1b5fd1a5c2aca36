"""One randomised differential case, GPU path (through the C ABI) vs the CPU oracle -- shared by
tests/test_gpu_soak.py (the driver's GPU suite runs 600 + a few large ones) and tools/soak.py (the
builder's longer campaigns): random n / split / bands, nk 2..11 (12..33: the wide-k tile kernel), sketchsize64 1..156, bbits in {14 (tile
kernel), 8, 16 (generic kernel)}, multi-cluster random tables in random or contiguous runs, related /
unrelated data, counts / jaccard / distance / fused-edge modes, neighbours from the tiles, both
settings of the two [EXT] switches (kernel and oracle flipped together), the four options of the coded copies
("rank_planes", "rank_short", "rank_fold", "rank_fold2") and, in half of the bbits 14 self cases, one to three positions planted with a
count of distinct or of shared values at a threshold of the coded copies' planes (128 | 129 ... 2 048 | 2 049).  A self job
that fits the coded route runs it once more at the end under every setting of "rank_fold" and "rank_short".
"""
import os

import numpy as np

from oracle import oracle
from poppunk_amd import _lib, engine, pp_sketchlib, synth


def reset_options():
    _lib.set_option("ext_collision_adjust", 0)
    _lib.set_option("ext_fit_skip", 0)
    _lib.set_option("ksplit", 1200)
    _lib.set_option("ksplit_slices", 0)
    _lib.set_option("ksplit_fused", 1)
    _lib.set_option("ks_grid_pad", 0)
    _lib.set_option("launch_tiles", 8000000)
    _lib.set_option("knn_list", 0)
    _lib.set_option("chunk_rows", 8 << 20)
    for name, default in (("wide_kpg", 0), ("lds_table", 1), ("ksplit_wide", 215), ("knn_warm", 32), ("knn_cut", 4),
                          ("ksplit_long", 1), ("host_parts", 2), ("host_parts_rows", 16 << 20), ("prefault_threads", 8), ("db_cache", 1),
                          ("progress", 1), ("host_trace", 0), ("rank_planes", 1), ("rank_short", 1), ("rank_fold", 1),
                          ("sweep_window", 1), ("knn_lane_lists", 0), ("ksplit_scratch_mb", 2048), ("rank_fold2", 1),
                          ("pairs_chunk", 0), ("pairs_scratch_mb", 1024)):
        _lib.set_option(name, default)
    oracle.set_ext(0, 0)


RANK_THRESHOLDS = (128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)      # either side of what decides a plane


def plant_position(sk, rng, s64, top=False):
    """One (k, bin) position of bbits = 14 sketches gets a count at a threshold of the coded copies, drawn from those n
    allows: either d distinct values spread over the samples (D = d), or d - 2 values with exactly two holders and single
    holders for the rest (E = S + 2 = d, D = n - d + 2).  Values and holders are drawn.  `top`: D one past the largest
    threshold n allows, i.e. the most planes a population of this size can take."""
    n, nk = sk.shape[0], sk.shape[1]
    fit = [d for d in RANK_THRESHOLDS if d <= n]
    if not fit:
        return None
    d = int(rng.choice(fit))
    shared = bool(rng.integers(0, 2)) and n - 2 * (d - 2) >= 1
    if top:
        d, shared = max(x for x in fit if x % 2), False
    idx = np.arange(n)
    if shared:
        idx[:2 * (d - 2)] %= d - 2
        idx[2 * (d - 2):] -= d - 2
    else:
        idx %= d
    vals = rng.permutation(1 << 14)[idx][rng.permutation(n)].astype(np.uint64)
    k, blk, bit = int(rng.integers(0, nk)), int(rng.integers(0, s64)), np.uint64(rng.integers(0, 64))
    for b in range(14):
        w = sk[:, k, blk * 14 + b]
        sk[:, k, blk * 14 + b] = (w & ~(np.uint64(1) << bit)) | (((vals >> np.uint64(b)) & np.uint64(1)) << bit)
    return "%s%d" % ("E" if shared else "D", d)


def route_label(kernel):
    """ppk_last_kernel_name() in short: the k-split forms, the wide-k tile kernel, the coded tile kernel with its planes
    ("rank 8", "rank 10 fold"), the raw tile kernel, the generic-bbits kernel"""
    if "rank " in kernel:
        return "rank %s%s" % (kernel.split("rank ")[1].split(",")[0].rstrip(">"),
                              " fold" if kernel.endswith("fold>") else " fold2" if kernel.endswith("fold2>") else "")
    return ("ksplit1" if "k-split fused" in kernel else "ksplit2" if "k-split counts" in kernel else
            "wide" if kernel.endswith("wide>") else "tile" if "256x32" in kernel else "generic")


def soak_case(rng, big=False):
    """Runs one case drawn from `rng`; returns (description, list of mismatch messages)."""
    import torch
    # draws added after the campaign was committed come from a child stream: `rng` gives every earlier draw as before
    extra = np.random.Generator(np.random.PCG64(rng.bit_generator.seed_seq.spawn(1)[0]))
    # ... and draws added after those from a child of that child: `extra` gives its draws as before, too
    later = np.random.Generator(np.random.PCG64(extra.bit_generator.seed_seq.spawn(1)[0]))
    bbits = int(rng.choice([14, 14, 14, 8, 16]))
    s64 = int(rng.choice([1, 2, 3, 16, 16, 16, 5, 40, 64, 156]))      # (32 and up: the long-sketch rule, k-split at any size)
    if os.environ.get("SOAK_KSPLIT"):      # the hand-over campaign: only shapes the one-launch k-split path takes
        bbits = 14
        s64 = int(rng.choice([2, 3, 16, 16, 16, 5, 40, 64, 156]))
    nk = int(rng.integers(2, 12))      # count registers of 2, 3 and 4 dwords
    wide_list = bbits == 14 and rng.integers(0, 5) == 0
    if wide_list:                      # the wide-k tile kernel: more than 128 count bits per pair
        nk = int(rng.integers(12, 34))
    k0 = int(rng.integers(9, 16)) if not wide_list else int(rng.integers(7, 12))
    kmers = (k0 + np.arange(nk) * (int(rng.integers(1, 5)) if not wide_list else int(rng.integers(1, 3)))).astype(np.int32)
    n = int(rng.integers(2, 1400 if s64 <= 16 else (500 if s64 <= 64 else 320)))
    if big:        # many ref tiles: the default-shape kernel at scale
        bbits, s64 = 14, 16
        n = int(rng.integers(2000, 7000))
    related = bool(rng.integers(0, 4))
    # half of the cases force the tile kernel's own epilogue (small jobs default to the k-split path)
    if rng.integers(0, 2):
        _lib.set_option("ksplit", 0)
    else:
        _lib.set_option("ksplit", 640)
    # small jobs: ONE launch (round 4) with every way of cutting a k into pieces, now and then the two-pass path
    _lib.set_option("ksplit_slices", int(rng.choice([0, 0, 1, 2, 4])))
    _lib.set_option("ksplit_fused", int(rng.integers(0, 8) != 0))
    # half of the cases put the units of a k-split tile on different XCDs (an odd grid width)
    _lib.set_option("ks_grid_pad", int(rng.integers(0, 2)))
    if os.environ.get("SOAK_KSPLIT"):
        # the hand-over campaign: every case a one-launch k-split job whose tiles' units run on DIFFERENT XCDs
        _lib.set_option("ksplit", 640)
        _lib.set_option("ksplit_fused", 1)
        _lib.set_option("ks_grid_pad", 1)
    _lib.set_option("ksplit_wide", int(rng.choice([215, 215, 0, 2000])))
    _lib.set_option("ksplit_long", int(rng.integers(0, 3) != 0))
    # every sixth case windows the count register narrower than it is (the wide-k path on short k lists); now and
    # then the LDS-table fit of interior tiles is off
    _lib.set_option("wide_kpg", int(rng.integers(1, 6)) if rng.integers(0, 6) == 0 else 0)
    _lib.set_option("lds_table", int(rng.integers(0, 6) != 0))
    # host-call plumbing (never changes results): staged neighbour opening / cuts, worker entries per device, page
    # pre-touching, the resident-database cache, progress meter and trace on fd 2
    _lib.set_option("knn_warm", int(rng.choice([32, 32, 0, 4])))
    _lib.set_option("knn_cut", int(rng.choice([4, 4, 0, 1])))
    _lib.set_option("host_parts", int(rng.choice([2, 2, 1, 3])))
    _lib.set_option("host_parts_rows", int(rng.choice([16 << 20, 16 << 20, 1, 5000])))
    _lib.set_option("prefault_threads", int(rng.choice([8, 8, 0, 3])))
    _lib.set_option("db_cache", int(rng.integers(0, 4) != 0))
    _lib.set_option("progress", int(rng.integers(0, 4) != 0))
    # the coded copies of a bbits = 14 database whose self job runs whole tiles (same bits either way)
    _lib.set_option("rank_planes", int(extra.choice([1, 1, 1, 0])))
    _lib.set_option("rank_short", int(extra.choice([1, 1, 0])))
    _lib.set_option("rank_fold", int(extra.choice([1, 1, 0, 2])))
    _lib.set_option("rank_fold2", int(later.choice([1, 1, 0, 2])))      # (2: the two-holder pair at any size the caps allow)
    # a quarter of the cases run as a very large job would: a few tiles per launch, a short neighbour-candidate
    # list, small pieces in the fused host call
    tiny = rng.integers(0, 4) == 0
    _lib.set_option("launch_tiles", int(rng.integers(2, 40)) if tiny else 8000000)
    _lib.set_option("knn_list", int(rng.integers(1, 1 << 16)) if tiny else 0)
    _lib.set_option("chunk_rows", int(rng.integers(16, 4096)) if tiny else 8 << 20)
    ext = (int(rng.integers(0, 2)), int(rng.integers(0, 2))) if rng.integers(0, 3) == 0 else (0, 0)
    _lib.set_option("ext_collision_adjust", ext[0])
    _lib.set_option("ext_fit_skip", ext[1])
    oracle.set_ext(ext[0], ext[1])
    sk, member = synth.make_sketches(n, kmers, sketchsize64=s64, bbits=bbits,
                                     cluster_size=int(rng.integers(5, 80)), seed=int(rng.integers(1, 1 << 30)),
                                     related=related)
    n_clu = int(rng.choice([1, 1, 2, 3]))
    tbl = (rng.random((nk, n_clu, n_clu)) * 0.05).astype(np.float32)
    clu = (rng.integers(0, n_clu, size=n)).astype(np.uint16)
    if rng.integers(0, 2):
        clu = np.sort(clu)          # contiguous runs: whole tiles with one cluster pair (the LDS-table epilogue)
    use_tbl = bool(rng.integers(0, 4))
    nr = int(rng.integers(1, n)) if n > 2 and rng.integers(0, 2) else n
    planted = []
    if bbits == 14 and nr == n and extra.integers(0, 2):
        planted = [plant_position(sk, extra, s64, top=i == 0) for i in range(int(extra.integers(1, 4)))]
    ref, qry = sk[:nr], (sk[nr:] if nr < n else None)
    rclu, qclu = clu[:nr], (clu[nr:] if nr < n else None)
    kw = dict(random_table=tbl if use_tbl else None, ref_clusters=rclu if use_tbl else None,
              qry_clusters=qclu if (use_tbl and qry is not None) else None, random_correct=use_tbl)
    okw = dict(random_tbl=tbl if use_tbl else None, ref_clu=rclu if use_tbl else None,
               qry_clu=qclu if (use_tbl and qry is not None) else None, random_correct=use_tbl, threads=8)
    msgs = []
    route = "-"
    import sys
    trace = (lambda what: (sys.stderr.write("soak: %s\n" % what), sys.stderr.flush())) if os.environ.get("SOAK_TRACE") \
        else (lambda what: None)
    trace("bbits=%d s64=%d nk=%d n=%d nr=%d clu=%d tbl=%d related=%d ext=%s tiny=%d ksplit=%d slices=%d fused=%d pad=%d" % (
        bbits, s64, nk, n, nr, n_clu, use_tbl, related, ext, tiny, _lib.get_option("ksplit"),
        _lib.get_option("ksplit_slices"), _lib.get_option("ksplit_fused"), _lib.get_option("ks_grid_pad")))
    try:
        c, _ = pp_sketchlib.query_arrays(ref, qry, kmers, s64, bbits, counts=True)
        trace("counts done")
        if not np.array_equal(c, oracle.match_counts(ref, qry, s64, bbits, threads=8)):
            msgs.append("counts differ")
        got, gf = pp_sketchlib.query_arrays(ref, qry, kmers, s64, bbits, **kw)
        route = route_label(_lib.lib().ppk_last_kernel_name().decode())
        trace("dist done")
        want, wf = oracle.query(ref, qry, kmers, s64, bbits, **okw)
        err = float(np.abs(got - want).max(initial=0))
        if gf != wf or not err <= 1e-6:
            msgs.append("dist: failed %d vs %d, max err %.3g" % (gf, wf, err))
        gj, _ = pp_sketchlib.query_arrays(ref, qry, kmers, s64, bbits, jaccard=True, **kw)
        wj, _ = oracle.query(ref, qry, kmers, s64, bbits, jaccard=True, **okw)
        if not np.abs(gj - wj).max(initial=0) <= 1e-6:
            msgs.append("jaccard differs")
        # bands + fused edges on the resident path
        db = engine.SketchDB(ref, s64, bbits, clusters=rclu if use_tbl else None)
        dbq = engine.SketchDB(qry, s64, bbits, clusters=qclu if use_tbl else None) if qry is not None else None
        nq = qry.shape[0] if qry is not None else nr
        cuts = sorted(set([0, nq] + [int(x) for x in rng.integers(0, nq + 1, size=3)]))
        t_tbl = tbl if use_tbl else None
        parts = [engine.dist(db, dbq, kmers, t_tbl, random_correct=use_tbl, q_begin=a, q_end=b)[0]
                 for a, b in zip(cuts[:-1], cuts[1:])]
        whole = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 2), np.float32)
        trace("bands done %s" % cuts)
        if not np.abs(whole - want).max(initial=0) <= 1e-6:
            msgs.append("bands differ")
        if want.shape[0]:
            slope = int(rng.integers(0, 3))
            x_max, y_max = synth.boundary_for_quantile(got, float(rng.uniform(0.05, 0.7)))
            inclusive = bool(rng.integers(0, 2))
            scale = (float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0)))
            scaled = (got / np.asarray(scale, dtype=np.float32)).astype(np.float32)
            we = oracle.edge_threshold(scaled, slope, x_max, y_max, n_ref=0 if qry is None else nr,
                                       inclusive=inclusive)
            # counts wider than 128 bits per pair at a bbits other than PopPUNK's 14 (the generic kernel): only the
            # whole matrix has an edge list (documented limit: a band is refused)
            cnt_bits = int(64 * s64).bit_length()
            ecuts = cuts if (nk * cnt_bits <= 128 or bbits == 14) else [0, nq]
            fe = [engine.dist_edges(db, dbq, kmers, t_tbl, random_correct=use_tbl, slope=slope, x_max=x_max,
                                    y_max=y_max, scale=scale, inclusive=inclusive, q_begin=a, q_end=b, cap=16)[0]
                  for a, b in zip(ecuts[:-1], ecuts[1:])]
            fe = torch.cat(fe).cpu().numpy()
            trace("fused edges done")
            if not np.array_equal(fe, np.asarray(we).reshape(-1, 2)):
                msgs.append("fused edges differ (%d vs %d)" % (len(fe), len(we)))
            # the same list as ONE host call (ppk_query_edges): the device listed 1 - 3 times when bands may
            # be cut, too little room now and then (the parked list is fetched)
            n_ent = int(rng.integers(1, 4)) if (nk * cnt_bits <= 128 or bbits == 14) else 1
            he, hf = pp_sketchlib.query_edges_arrays(ref, qry, kmers, s64, bbits, slope, x_max, y_max, scale=scale,
                                                     inclusive=inclusive, random_table=t_tbl,
                                                     ref_clusters=rclu if use_tbl else None,
                                                     qry_clusters=qclu if use_tbl and qry is not None else None,
                                                     random_correct=use_tbl, devices=(0,) * n_ent,
                                                     cap=3 if rng.integers(0, 4) == 0 else None)
            if hf != gf or not np.array_equal(he, np.asarray(we).reshape(-1, 2)):
                msgs.append("host fused edges differ (%d vs %d, %d entries)" % (len(he), len(we), n_ent))
        # neighbours straight from the tiles == get_kNN_distances(longToSquare(.)) of the same distances
        cnt_bits_k = int(64 * s64).bit_length()
        if qry is None and bbits == 14 and nr > 1:
            knn = int(rng.integers(1, 33))
            col = int(rng.integers(0, 2))
            gi, gj, gd = engine.knn_from_sketches(db, kmers, t_tbl, knn, dist_col=col, random_correct=use_tbl,
                                                  method="tiles")
            wi, wj, wd = oracle.knn(oracle.long_to_square(got[:, col]), knn)
            if not (np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gj.cpu().numpy(), wj)
                    and np.array_equal(gd.cpu().numpy(), wd)):
                msgs.append("kNN from tiles differs (k=%d col=%d)" % (knn, col))
        # ref x query: every ref's nearest queries and every query's nearest refs from one pass over the rectangle
        if qry is not None and bbits == 14:
            knn = int(rng.integers(1, 33))
            col = int(rng.integers(0, 2))
            gi, gj, gd = (x.cpu().numpy() for x in engine.knn_ref_query(db, dbq, kmers, t_tbl, knn, dist_col=col,
                                                                        random_correct=use_tbl))
            rect = got[:, col].reshape(nq, nr)                      # row = q * n_ref + r
            wj = np.zeros((nr + nq, knn), dtype=np.int64)
            wd = np.zeros((nr + nq, knn), dtype=np.float32)
            for r in range(nr):
                o = np.argsort(rect[:, r], kind="stable")[:knn]
                wj[r, :len(o)], wd[r, :len(o)] = o + nr, rect[o, r]
            for q in range(nq):
                o = np.argsort(rect[q], kind="stable")[:knn]
                wj[nr + q, :len(o)], wd[nr + q, :len(o)] = o, rect[q, o]
            if not (np.array_equal(gi, np.repeat(np.arange(nr + nq), knn)) and np.array_equal(gj, wj.ravel())
                    and np.array_equal(gd, wd.ravel())):
                msgs.append("ref x query kNN from tiles differs (k=%d col=%d)" % (knn, col))
        # the coded copies, whatever route the case's own options gave its jobs: a self job whose counts fit 64 bits runs
        # whole tiles with the k-split path off, on a database created under each "rank_fold" and launched under both
        # "rank_short" (the three large cases run s64 = 16 alone, where the directed tests sit)
        coded = set()
        if qry is None and not big and bbits == 14 and nr > 1 and nk * cnt_bits_k <= 64 and _lib.get_option("rank_planes"):
            saved = {name: _lib.get_option(name) for name in ("ksplit", "ksplit_long", "wide_kpg", "rank_fold", "rank_short")}
            for name in ("ksplit", "ksplit_long", "wide_kpg"):
                _lib.set_option(name, 0)
            for fold in (0, 1, 2):
                _lib.set_option("rank_fold", fold)
                dbc = engine.SketchDB(ref, s64, bbits, clusters=rclu if use_tbl else None)
                for short in (1, 0):
                    _lib.set_option("rank_short", short)
                    cd = engine.dist(dbc, None, kmers, t_tbl, random_correct=use_tbl)[0].cpu().numpy()
                    coded.add(route_label(_lib.lib().ppk_last_kernel_name().decode()))
                    if not np.abs(cd - want).max(initial=0) <= 1e-6:
                        msgs.append("coded self job differs (rank_fold %d rank_short %d)" % (fold, short))
                dbc.close()
            for name, value in saved.items():
                _lib.set_option(name, value)
            route += " +" + "/".join(sorted(coded))
        db.close()
        if dbq is not None:
            dbq.close()
    except Exception as e:  # noqa: BLE001
        msgs.append("EXCEPTION %r" % (e,))
    desc = ("bbits=%2d s64=%2d nk=%d n=%4d nr=%4d clu=%d tbl=%d related=%d ext=%d%d tiny=%d pad=%d %s"
            " rank_planes=%d rank_short=%d rank_fold=%d rank_fold2=%d planted=%s"
            % (bbits, s64, nk, n, nr, n_clu, use_tbl, related, ext[0], ext[1], int(tiny), _lib.get_option("ks_grid_pad"),
               route, _lib.get_option("rank_planes"), _lib.get_option("rank_short"), _lib.get_option("rank_fold"),
               _lib.get_option("rank_fold2"), ",".join(x for x in planted if x) or "-"))
    return desc, msgs
