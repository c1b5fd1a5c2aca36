"""Embeddings on the device (ppk_embed_weights_dev, ppk_embed_dev, engine.embed*, mandrake): P to
rounding and Y bit for bit against the restatement (tests/test_embed_host.py), repeatability, every input form, bad
entries, and the quality gates from sketches.  Sizes are bounded (n <= 100 000, at most 1 000 iterations), so a
wrong kernel fails rather than hangs."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import engine, mandrake, poppunk_refine, synth  # noqa: E402
from test_embed_host import (OVERLAP_GATE, SAME_GATE, calibrate, embed, knn_lists, planted,  # noqa: E402
                             quality, schedule, weights)

DEV = "cuda:0"
SAME_GATE_100K = 0.75      # 100 000 genomes, K = 30 from the tiles path: 0.79 reached


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def cuda(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device=DEV)


def lists(n, k, seed):
    D, labels = planted(nc=max(2, n // 100), size=100, seed=seed) if n >= 200 else planted(nc=2, size=n // 2,
                                                                                           seed=seed)
    D = D[:n, :n]
    return knn_lists(D, k), labels[:n]


def device_weights(i, j, d, n, perp=20.0):
    P, c = engine.embed_weights_dev(cuda(i, np.int64), cuda(j, np.int64), cuda(d, np.float32), n, perp,
                                    weights=True)
    return P.cpu().numpy(), c.cpu().numpy().view(np.uint64)


def device_embed(i, j, P, n, seed, max_iter, workers=65536):
    Y = engine.embed_dev(cuda(i, np.int64), cuda(j, np.int64), cuda(P, np.float64), n, seed, max_iter=max_iter,
                         workers=workers)
    return Y.cpu().numpy()


def embedded_knn_dev(Y, k=10):
    """the k nearest embedded neighbours of every point, on the device (chunks of 2048 rows)"""
    Yt = torch.as_tensor(Y, device=DEV)
    out = []
    for s in range(0, Yt.shape[0], 2048):
        d = torch.cdist(Yt[s:s + 2048], Yt)
        d[torch.arange(d.shape[0]), torch.arange(s, s + d.shape[0])] = float("inf")
        out.append(torch.topk(d, k, largest=False).indices)
    return torch.cat(out).cpu().numpy()


@pytest.mark.parametrize("n,k,perp", [(50, 20, 5.0), (500, 50, 20.0), (300, 9, 20.0)])
def test_weights_match_the_restatement(n, k, perp):
    (i, j, d), _ = lists(n, k, seed=n)
    P, c = device_weights(i, j, d, n, perp)
    want = calibrate(d, n, k, perp)
    assert np.allclose(P, want, rtol=1e-12, atol=0)
    assert np.array_equal(c, weights(P))
    assert abs(P.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("n,max_iter,workers", [(50, 20000, 65536), (500, 200000, 65536), (500, 30000, 64),
                                                (5000, 100000, 65536), (5000, 60000, 1024)])
def test_bit_for_bit(n, max_iter, workers):
    (i, j, d), _ = lists(n, min(50, n - 1), seed=n + 1)
    k = min(50, n - 1)
    P, _ = device_weights(i, j, d, n)
    assert schedule(n, max_iter, workers)[1] <= 2000
    Y = device_embed(i, j, P, n, seed=1234 + n, max_iter=max_iter, workers=workers)
    want = embed(P, i, j, n, seed=1234 + n, max_iter=max_iter, workers=workers)
    assert np.all(np.isfinite(Y))
    assert np.array_equal(bits(Y), bits(want))
    assert k == len(i) // n


def test_two_runs_same_bits():
    (i, j, d), _ = lists(2000, 50, seed=4)
    P, _ = device_weights(i, j, d, 2000)
    a = device_embed(i, j, P, 2000, seed=5, max_iter=10 ** 6)
    b = device_embed(i, j, P, 2000, seed=5, max_iter=10 ** 6)
    assert np.array_equal(bits(a), bits(b))
    c = device_embed(i, j, P, 2000, seed=6, max_iter=10 ** 6)
    assert not np.array_equal(bits(a), bits(c))


@pytest.fixture(scope="module")
def sketches_2000():
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, labels = synth.make_sketches(2000, kmers, cluster_size=50, seed=17)
    db = engine.SketchDB(sk, 16, 14, device=0)
    yield db, kmers, tbl, labels
    db.close()


def test_every_input_form_same_y(sketches_2000):
    db, kmers, tbl, _ = sketches_2000
    n, K, mi = 2000, 30, 200000
    for method in ("square", "tiles"):
        i, j, d = engine.knn_from_sketches(db, kmers, tbl, K, dist_col=1, method=method)
        P = engine.embed_weights_dev(i, j, d, n, 20.0)
        Y_dev = engine.embed_dev(i, j, P, n, 77, max_iter=mi).cpu().numpy()
        Ph, Y_host = engine.embed(i.cpu().numpy(), j.cpu().numpy(), d.cpu().numpy(), n, 77, max_iter=mi)
        assert np.array_equal(bits(Ph), bits(P.cpu().numpy()))
        assert np.array_equal(bits(Y_dev), bits(Y_host))
        if method == "square":
            Y_square = Y_dev
            # the same lists through poppunk_refine.get_kNN_distances of the host square
            tri, _ = engine.dist(db, None, kmers, tbl)
            sq = engine.long_to_square_dev(tri, 1, n).cpu().numpy()
            I, J, Dl = poppunk_refine.get_kNN_distances(sq, K, 1)
            assert np.array_equal(np.asarray(J), j.cpu().numpy())
            _, Y_sq = engine.embed(I, J, Dl, n, 77, max_iter=mi)
            assert np.array_equal(bits(Y_sq), bits(Y_square))
        elif np.array_equal(d.cpu().numpy(), Dl) and np.array_equal(j.cpu().numpy(), np.asarray(J)):
            assert np.array_equal(bits(Y_dev), bits(Y_square))      # the same lists from the tiles


@pytest.mark.parametrize("bad", ["nan", "negative", "j_range", "j_self", "ungrouped"])
def test_bad_entries_named(bad):
    (i, j, d), _ = lists(200, 10, seed=3)
    i, j, d = i.copy(), j.copy(), d.copy()
    e = 537
    if bad == "nan":
        d[e] = np.nan
    elif bad == "negative":
        d[e] = -1.0
    elif bad == "j_range":
        j[e] = 200
    elif bad == "j_self":
        j[e] = i[e]
    else:
        i[e] = i[e] + 1
    with pytest.raises(RuntimeError) as ex:
        device_weights(i, j, d, 200)
    msg = str(ex.value)
    assert "entry 537" in msg, msg
    want = {"nan": "NaN", "negative": "negative", "j_range": "outside", "j_self": "j = i", "ungrouped": "grouped"}
    assert want[bad] in msg, msg
    if bad in ("j_range", "j_self", "ungrouped"):
        P = np.full(len(i), 1.0 / len(i))
        with pytest.raises(RuntimeError) as ex:
            device_embed(i, j, P, 200, seed=1, max_iter=1000)
        assert "entry 537" in str(ex.value) and want[bad] in str(ex.value)
    (i, j, d), _ = lists(200, 10, seed=3)
    P = np.full(len(i), 1.0 / len(i))
    P[e] = np.nan
    with pytest.raises(RuntimeError) as ex:
        device_embed(i, j, P, 200, seed=1, max_iter=1000)
    assert "entry 537" in str(ex.value) and "NaN" in str(ex.value)


def test_generate_embedding_small_n_and_file(tmp_path):
    D = np.array([[0, 1, 2], [1, 0, 1.5], [2, 1.5, 0]], dtype=np.float32)
    out = tmp_path / "p"
    out.mkdir()
    fn = mandrake.generate_embedding(["a", "b", "c"], D, 20, str(out), False, maxIter=30000, seed=3)
    text = open(fn).read()
    assert text.startswith('graph G { "a"[x="') and text.endswith("}\n") and text.count("];") == 3
    fn2 = mandrake.generate_embedding(["a", "b"], D[:2, :2].copy(), 20, str(out), True, kNN=100, maxIter=20000,
                                      seed=3)
    assert fn2 == fn and open(fn).read().count("];") == 2


def sketch_run(n, knn, seed, method="auto", max_iter=10000000):
    """(Y, neighbour j, labels, wall seconds of sketches -> Y) for the device population model of n genomes"""
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    db = engine.SketchDB(synth.make_sketches_device(n, kmers, seed=seed), 16, 14, device=0)
    try:
        torch.cuda.synchronize()
        t0 = time.time()
        Y = mandrake.embed_sketches(db, kmers, tbl, 20.0, kNN=knn, maxIter=max_iter, seed=seed,
                                   method=method).cpu().numpy()
        wall = time.time() - t0
        _, j, _ = engine.knn_from_sketches(db, kmers, tbl, knn, dist_col=1, method=method)
    finally:
        db.close()
    return Y, j.cpu().numpy(), np.arange(n) % (n // 50), wall


def test_quality_10000_from_sketches():
    Y, j, labels, wall = sketch_run(10000, 50, seed=23)
    assert np.all(np.isfinite(Y)) and wall < 120, wall
    same, overlap = quality(embedded_knn_dev(Y), labels, j, 50)
    print("n = 10000: same-cluster %.4f, overlap %.4f, %.2f s" % (same, overlap, wall))
    assert same >= SAME_GATE and overlap >= OVERLAP_GATE, (same, overlap)


def test_100000_from_sketches_tiles():
    # 2 * 10^8 samples; at the default 10^7 (153 iterations of 65 536 workers) 100 000 genomes are under-converged,
    # and from 2 * 10^8 to 10^9 the measures hold at about 0.80 and 0.19: this size has its own gate
    Y, j, labels, wall = sketch_run(100000, 30, seed=31, method="tiles", max_iter=2 * 10 ** 8)
    assert np.all(np.isfinite(Y))
    assert wall < 120, wall
    same, overlap = quality(embedded_knn_dev(Y), labels, j, 30)
    print("n = 100000: same-cluster %.4f, overlap %.4f, %.2f s" % (same, overlap, wall))
    assert same >= SAME_GATE_100K and overlap >= OVERLAP_GATE, (same, overlap)
