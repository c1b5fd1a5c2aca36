#!/usr/bin/env python3
"""Pin kit: settle the embedding against mandrake's SCE.wtsne.

poppunk_amd's embedding restates mandrake's stochastic cluster embedding as recalled; mandrake is not installed where
this library is built, so the rules marked [EXT] in DESIGN.md 3.11 are pinned by nothing there.  Wherever SCE and
this package with an MI355X are both importable, this script embeds the same neighbour lists (20 planted Gaussian
clusters of 100 samples, K = 50, perplexity 20) with SCE.wtsne (mandrake.py:95-107's call, one worker) and with
engine.embed, and compares the quality measures of DESIGN.md 3.11, not the coordinates (the generators differ):

  - the fraction of each point's 10 nearest embedded neighbours that share its cluster;
  - the overlap of those neighbours with its 10 nearest input neighbours.

    python tools/pin_mandrake.py [--device N] [--max-iter M]

Exit status 0 = both measures of this package within 0.05 of SCE's or above them, 1 = below, 2 = SCE not
importable (nothing pinned).  It is EXPECTED to exit 2 in the build container and on the GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=10 ** 6)
    a = ap.parse_args()
    try:
        from SCE import wtsne
    except ImportError:
        print("SCE (mandrake) is not importable: nothing pinned")
        return 2
    from poppunk_amd import engine
    from test_embed_host import embedded_neighbours, knn_lists, planted, quality
    D, labels = planted()
    n, K = D.shape[0], 50
    i, j, d = knn_lists(D, K)
    res = wtsne(i.tolist(), j.tolist(), d.tolist(), np.ones(n), perplexity=20, maxIter=a.max_iter, nRepuSamp=5,
                eta0=1, bInit=0, animated=False, n_workers=1, n_threads=1, seed=1)
    Y_ref = np.array(res.get_embedding()).reshape(-1, 2)
    _, Y = engine.embed(i, j, d, n, 1, perplexity=20.0, max_iter=a.max_iter, device_id=a.device)
    ref = quality(embedded_neighbours(Y_ref), labels, j, K)
    got = quality(embedded_neighbours(Y), labels, j, K)
    print("SCE.wtsne:   same-cluster %.4f, overlap %.4f" % ref)
    print("ppk_embed:   same-cluster %.4f, overlap %.4f" % got)
    ok = all(g >= r - 0.05 for g, r in zip(got, ref))
    print("within 0.05 or above: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
