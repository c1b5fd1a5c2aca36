"""GPU test of `python -m poppunk_amd.reference_pick` (poppunk_references), in process: a synthetic
database, its distances, network file and model directory in; the .refs file, the reference network, the pruned
distances, the pruned sketch database and the copied model files out, each checked against what went in."""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import refs_model as rm  # noqa: E402
from poppunk_amd import poppunk_refine, pp_sketchlib, reference_pick, sketchdb, synth  # noqa: E402
from poppunk_amd.distfile import readPickle, storePickle  # noqa: E402


def test_command_line_end_to_end(tmp_path, capsys):
    n = 120
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(n, kmers, cluster_size=30, seed=5)
    names = ["iso_%03d" % k for k in range(n)]
    dist, _ = pp_sketchlib.query_arrays(sk, None, kmers, 16, 14, tbl)
    x_max, y_max = synth.boundary_for_quantile(dist, 0.15)
    edges = poppunk_refine.edgeThreshold_array(dist, 2, x_max, y_max)

    db = str(tmp_path / "full")
    sketchdb.save_h5(db + "/full", names, kmers, sk, 16, 14, random_table=tbl, clusters=np.zeros(n, dtype=np.uint16))
    storePickle(names, names, True, dist, db + "/full.dists")
    np.savez(db + "/full_graph.npz", edges=edges, n_vertices=n)
    model = str(tmp_path / "fit")
    os.makedirs(model)
    for ending, text in (("_fit.pkl", b"pkl"), ("_fit.npz", b"npz"), ("_clusters.csv", b"Taxon,Cluster\n")):
        open(model + "/fit" + ending, "wb").write(text)
    out = str(tmp_path / "picked")

    with pytest.raises(SystemExit) as done:
        reference_pick.main(["--network", db + "/full_graph.npz", "--distances", db + "/full.dists", "--ref-db", db,
                             "--model", model, "--output", out, "--threads", "2"])
    assert done.value.code == 0
    err = capsys.readouterr().err
    assert "Network loaded: 120 samples\n" in err and "Running clique finding\n" in err

    want, want_edges, _ = rm.pick_refs(edges, n)
    idx = np.flatnonzero(want)
    ref_names = [names[k] for k in idx]
    assert 0 < len(idx) < n
    assert open(out + "/picked.refs").read() == "".join(s + "\n" for s in ref_names)
    g_edges, g_n = reference_pick.load_network_npz(out + "/picked.refs_graph.npz")
    assert g_n == len(idx) and np.array_equal(g_edges, want_edges)
    rlist, qlist, self_, pruned = readPickle(out + "/picked.dists", enforce_self=True)
    assert rlist == ref_names and qlist == ref_names and self_
    iu = np.triu_indices(n, 1)
    kept = want[iu[0]].astype(bool) & want[iu[1]].astype(bool)
    assert np.array_equal(pruned, dist[kept])                 # row order of the long form is kept
    assert sketchdb.getSeqsInDb(out + "/picked.h5") == ref_names and not os.path.exists(out + "/picked.tmp.h5")
    assert open(out + "/picked_fit.pkl", "rb").read() == b"pkl" and open(out + "/picked_fit.npz", "rb").read() == b"npz"
    assert open(out + "/picked_clusters.csv", "rb").read() == b"Taxon,Cluster\n"
    with open(out + "/picked.dists.pkl", "rb") as f:
        assert pickle.load(f)[2] is True
