#!/usr/bin/env python3
"""Generates tests/golden/refine_fit.npz: refine.refineFit as the reference computes it, step by step.

Run in the BUILD container only (needs the reference checkout, networkx, pandas and scipy); the fixture it writes is
data (lines, score lists, evaluated positions, counts, results) and is committed, the reference is not.

Reference code executed (pulled out of its modules with `ast`, as make_golden_network.py does, and run unmodified):
  PopPUNK/refine.py   refineFit, newNetwork, newNetwork2D, growNetwork, check_search_range
  PopPUNK/utils.py    transformLine, decisionBoundary
  PopPUNK/network.py  construct_network_from_df, construct_network_from_edge_list, networkSummary
under the real numpy / pandas / scipy of this image, make_golden_network.py's networkx stand-in for graph-tool, the
oracle's threshold_iterate_1d / _2d / edge_threshold in the place of poppunk_refine, and serial stand-ins for the
process pool and the shared memory of the unconstrained search (one process, one array).

The two distance matrices are those of network_sweep.npz (sweep1d_dist, n = 300; sweep2d_dist, n = 200), divided by
their column maxima as RefineFit.fit scales them; the fixture stores lines, not matrices.  Per case `<case>_...`:
  dist (the key in network_sweep.npz), scale, mean0, mean1, max_move, min_move, slope, unconstrained, no_local
  global_s   the global step's scores after NaN -> 1 (40, or the flattened 20 x 20 grid)
  bounds     [lo, hi] handed to scipy, or empty when no local step ran
  eval_s, eval_stats int64 [k, 4] (edges, components, triangles, connected triples), eval_score: every position
             scipy evaluated, in order, with the counts and the score (-networkSummary's) of that graph
  result     (optimal_x, optimal_y, optimised_s), or empty when the call raised; error = the RuntimeError's text
`tl_*` / `db_*`: inputs and outputs of transformLine / decisionBoundary (with and without adj).
"""
import os
import sys
from functools import partial
from itertools import chain

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_network import REF, _FakeGt, _Tqdm, extract_functions      # noqa: E402


class _Gt(_FakeGt):
    @staticmethod
    def openmp_enabled():
        return False


class _NumpyShared:
    def __init__(self, name, shape, dtype):
        self.name, self.shape, self.dtype = name, shape, dtype


class _Shm:
    """one process: a named bytearray"""
    blocks = {}

    def __init__(self, name=None, size=0):
        if name is None:
            name = "blk%d" % len(_Shm.blocks)
            _Shm.blocks[name] = bytearray(size)
        self.name, self.buf = name, _Shm.blocks[name]


class _Smm:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _Shm.blocks.clear()
        return False

    def SharedMemory(self, size):
        return _Shm(size=size)


class _SharedMemoryModule:
    SharedMemory = _Shm


class _Pool:
    def __init__(self, processes=1):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def map(self, fn, it):
        return [fn(x) for x in it]


def graph_counts(G):
    import networkx as nx
    g = G.g
    return [g.number_of_edges(), nx.number_connected_components(g), sum(nx.triangles(g).values()) // 3,
            sum(d * (d - 1) // 2 for _, d in g.degree())]


def reference_namespace(rec):
    import pandas as pd
    import scipy.optimize
    from oracle import oracle

    class _Refine:
        @staticmethod
        def thresholdIterate1D(distMat, s_range, slope, x0, y0, x1, y1, num_processes=1):
            return oracle.threshold_iterate_1d(distMat, s_range, slope, x0, y0, x1, y1)

        @staticmethod
        def thresholdIterate2D(distMat, x_range, y_max):
            return oracle.threshold_iterate_2d(distMat, x_range, y_max)

        @staticmethod
        def edgeThreshold(distMat, slope, x_max, y_max):
            return oracle.edge_threshold(distMat, slope, x_max, y_max)

    class _Optimize:
        @staticmethod
        def minimize_scalar(fun, bounds=None, **kw):
            rec["bounds"] = [float(bounds[0]), float(bounds[1])]
            return scipy.optimize.minimize_scalar(fun, bounds=bounds, **kw)

    class _Scipy:
        optimize = _Optimize

    ns = {"np": np, "pd": pd, "gt": _Gt, "tqdm": _Tqdm, "os": os, "sys": sys, "scipy": _Scipy, "chain": chain,
          "partial": partial, "poppunk_refine": _Refine, "NumpyShared": _NumpyShared, "shared_memory": _SharedMemoryModule,
          "SharedMemoryManager": _Smm, "Pool": _Pool, "betweenness_sample_default": 100}
    extract_functions(os.path.join(REF, "PopPUNK", "network.py"),
                      ["construct_network_from_df", "construct_network_from_edge_list", "networkSummary"], ns)
    extract_functions(os.path.join(REF, "PopPUNK", "utils.py"), ["transformLine", "decisionBoundary"], ns)
    extract_functions(os.path.join(REF, "PopPUNK", "refine.py"),
                      ["refineFit", "newNetwork", "newNetwork2D", "growNetwork", "check_search_range"], ns)
    summary, new_network, grow = ns["networkSummary"], ns["newNetwork"], ns["growNetwork"]

    def recording_summary(G, *a, **kw):
        out = summary(G, *a, **kw)
        if rec.get("in_eval"):
            rec["eval_stats"].append(graph_counts(G))
        return out

    def recording_new_network(s, *a, **kw):
        rec["in_eval"] = True
        score = new_network(s, *a, **kw)
        rec["in_eval"] = False
        rec["eval_s"].append(float(s))
        rec["eval_score"].append(float(score))
        return score

    def recording_grow(*a, **kw):
        scores = grow(*a, **kw)
        rec["grown"].append(list(scores))
        return scores

    ns["networkSummary"] = recording_summary
    ns["newNetwork"] = recording_new_network
    ns["growNetwork"] = recording_grow
    return ns


def run_case(dist, key, scale, mean0, mean1, max_move, min_move, slope=2, unconstrained=False, no_local=False,
             want_local=None, want_error=None):
    rec = {"eval_s": [], "eval_stats": [], "eval_score": [], "grown": [], "bounds": None}
    ns = reference_namespace(rec)
    n = int(round((1 + (1 + 8 * dist.shape[0]) ** 0.5) / 2))
    names = ["s%d" % k for k in range(n)]
    out = {"dist": np.array(key), "scale": scale, "mean0": np.array(mean0, dtype=np.float64),
           "mean1": np.array(mean1, dtype=np.float64), "max_move": np.float64(max_move), "min_move": np.float64(min_move),
           "slope": np.int64(slope), "unconstrained": np.bool_(unconstrained), "no_local": np.bool_(no_local)}
    error, result = "", np.zeros(0)
    try:
        res = ns["refineFit"](dist, names, np.array(mean0, dtype=np.float64), np.array(mean1, dtype=np.float64), scale,
                              max_move, min_move, slope=slope, unconstrained=unconstrained, no_local=no_local)
        result = np.array([float(v) for v in res], dtype=np.float64)
    except RuntimeError as e:
        error = str(e)
    if unconstrained:
        # newNetwork2D's rows: growNetwork's list, or the zeros of a boundary that lists every row (not recorded here:
        # the cases below are checked to have none)
        assert error or len(rec["grown"]) == 20, len(rec["grown"])
    global_s = np.array(list(chain.from_iterable(rec["grown"])), dtype=np.float64)
    global_s[np.isnan(global_s)] = 1
    ran_local = rec["bounds"] is not None
    if want_local is not None:
        assert ran_local == want_local, "local step: wanted %s, got %s (argmin %s of %d)" % (
            want_local, ran_local, np.argmin(global_s) if global_s.size else None, global_s.size)
    if want_error is not None:
        assert error == want_error, (error, want_error)
    else:
        assert not error, error
    out.update(global_s=global_s, bounds=np.array(rec["bounds"] if ran_local else [], dtype=np.float64),
               eval_s=np.array(rec["eval_s"], dtype=np.float64),
               eval_stats=np.array(rec["eval_stats"], dtype=np.int64).reshape(-1, 4),
               eval_score=np.array(rec["eval_score"], dtype=np.float64), result=result, error=np.array(error))
    return out


def main():
    sweep = np.load(os.path.join(HERE, "network_sweep.npz"))
    out, cases = {}, []
    mats = {}
    for key in ("sweep1d_dist", "sweep2d_dist"):
        d = sweep[key]
        scale = np.amax(d, axis=0)
        mats[key] = ((d / scale).astype(np.float32), scale)

    def add(name, key, *a, **kw):
        d, scale = mats[key]
        res = run_case(d, key, scale, *a, **kw)
        cases.append(name)
        for k, v in res.items():
            out["%s_%s" % (name, k)] = v
        print(name, "global", res["global_s"].size, "argmin", int(np.argmin(res["global_s"])) if res["global_s"].size else None,
              "bounds", res["bounds"], "evals", res["eval_s"].size, "result", res["result"], "error", repr(str(res["error"])))

    a, b = "sweep1d_dist", "sweep2d_dist"
    add("slope2_local", a, (0.08, 0.06), (0.55, 0.45), 0.05, 0.04, want_local=True)
    add("slope0_local", a, (0.08, 0.06), (0.55, 0.45), 0.05, 0.04, slope=0, want_local=True)
    add("slope1_local", a, (0.08, 0.06), (0.55, 0.45), 0.05, 0.04, slope=1, want_local=True)
    add("slope2_b_local", b, (0.08, 0.06), (0.55, 0.45), 0.05, 0.04, want_local=True)
    add("no_local", a, (0.08, 0.06), (0.55, 0.45), 0.05, 0.04, no_local=True, want_local=False)
    add("min_at_end", a, (0.02, 0.015), (0.08, 0.06), 0.0, 0.01, want_local=False)
    add("unconstrained_local", b, (0.08, 0.06), (0.55, 0.45), 0.05, 0.04, unconstrained=True, want_local=True)
    add("unconstrained_edge", b, (0.2, 0.2), (0.6, 0.6), 0.0, 0.05, unconstrained=True, want_local=False)
    add("below_zero", a, (0.08, 0.06), (0.55, 0.45), 0.05, 0.3, want_local=False, want_error="Boundary range below zero")
    add("all_points", a, (0.08, 0.06), (0.55, 0.45), 3.0, 0.04, want_local=False,
        want_error="Boundary range includes all points")

    # transformLine / decisionBoundary at a few points (decisionBoundary with adj changes its argument: both recorded)
    ns = reference_namespace({})
    rng = np.random.default_rng(7)
    tl_in = np.column_stack([rng.uniform(-0.2, 0.8, 12), rng.uniform(0, 0.3, (12, 2)), rng.uniform(0.4, 0.9, (12, 2))])
    tl_out = np.array([ns["transformLine"](r[0], r[1:3], r[3:5]) for r in tl_in])
    db_in = np.column_stack([rng.uniform(0.05, 0.6, (12, 2)), rng.uniform(0.3, 3.0, 12), rng.uniform(-0.04, 0.04, 12)])
    db_in[:4, 3] = 0.0
    db_out, db_after = [], []
    for r in db_in:
        p = r[0:2].copy()
        db_out.append(ns["decisionBoundary"](p, r[2], adj=r[3]))
        db_after.append(p)
    out.update(tl_in=tl_in, tl_out=tl_out, db_in=db_in, db_out=np.array(db_out, dtype=np.float64),
               db_after=np.array(db_after, dtype=np.float64))

    out["cases"] = np.array(cases)
    np.savez_compressed(os.path.join(HERE, "refine_fit.npz"), **out)


if __name__ == "__main__":
    main()
