"""GPU tests of reference picking (ppk_pick_refs*, engine.pick_references*, network.extractReferences):
the device against the numpy restatement of tests/refs_model.py, bit for bit (flags, renumbered reference edges and
all eight counts), and the independent property checker (P1-P3) on the device's output.  Fixed graphs, every stream
form, fast mode, the errors by message, the host twin, planted random graphs, and the pick used end to end: every
non-reference assigned back against the reference database gives the full graph's partition."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import refs_model as rm  # noqa: E402
from poppunk_amd import _lib, assign, engine, models, network, synth  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def edge_array(e):
    return np.asarray(e, dtype=np.int64).reshape(-1, 2)


def on_device(e, n, existing=None, merged=None, fast=False):
    r, re, c = engine.pick_references_dev(dev(edge_array(e)), n, None if existing is None else dev(existing),
                                          None if merged is None else dev(merged), fast)
    return r.cpu().numpy(), re.cpu().numpy(), c


def agree(e, n, existing=None, merged=None, fast=False):
    """device == restatement, and the properties on the device's output; -> (is_ref, ref_edges, counts)"""
    e = edge_array(e)
    got = on_device(e, n, existing, merged, fast)
    want = rm.pick_refs(e, n, existing, merged, fast)
    assert got[2] == want[2]
    assert np.array_equal(got[0], want[0]) and got[0].dtype == np.uint8
    assert np.array_equal(got[1], want[1]) and got[1].shape == want[1].shape
    assert rm.check_properties(e, n, got[0], got[1], clique_mode=not fast) == []
    return got


# ---- fixed graphs ----------------------------------------------------------------------------------------------------

def test_one_clique_of_200_gives_its_lowest_vertex():
    r, re, c = agree(rm.clique(200), 200)
    assert np.flatnonzero(r).tolist() == [0] and c["cliques_removed"] == 1 and len(re) == 0


def test_300_isolated_vertices_are_all_references():
    r, _, c = agree([], 300)
    assert r.all() and c["from_small"] == 300 and c["components"] == 300


@pytest.mark.parametrize("centre_lowest", [True, False])
def test_star_of_100_leaves(centre_lowest):
    r, _, c = agree(rm.star(100, centre_lowest), 101)
    # centre lowest: {centre, first leaf} goes first and gives the centre, the other 99 leaves are singleton leftovers
    # and references next to it; centre highest: {leaf 0, centre} gives leaf 0, the other leaves are singleton
    # leftovers, and the repair joins all of them through the centre
    assert c["cliques_removed"] == 100 and c["references"] == (100 if centre_lowest else 101)


def test_path_of_200_takes_references_from_leftovers_and_repairs():
    r, _, c = agree(rm.path(200), 200)
    assert c["cliques_removed"] == 100 and c["components_repaired"] == 1 and r[0] == 1


def test_dumbbell_needs_repair():
    e, n = rm.dumbbell()
    r, _, c = agree(e, n)
    assert c["components_repaired"] == 1 and c["added_by_repair"] > 0


def test_existing_references_suppress_every_new_pick():
    e, n = rm.shifted([(rm.clique(30), 30), (rm.clique(70), 70)])
    existing = np.zeros(n, dtype=np.uint8)
    existing[[17, 30 + 69]] = 1
    r, _, c = agree(e, n, existing)
    assert np.array_equal(r, existing) and c["from_cliques"] == 0 and c["references"] == 2


def test_existing_references_five_hops_apart_are_joined():
    # "the repair adds the 4 between them": under the rule the pruning comes first and already picks one of the four
    # (path 0-1-2-3-4-5: {0, 1} and {4, 5} hold an existing reference, {2, 3} holds none, so 2 is picked), and the
    # repair adds the other three.  What is asserted is that all four come out as references, by those two routes
    # together, and nothing else is added -- not less than "4 between them" asks.
    e, n, existing = rm.far_existing(5)
    r, _, c = agree(e, n, existing)
    assert r.all() and c["from_cliques"] + c["added_by_repair"] == 4 and c["components_repaired"] == 1


def test_three_components_repaired_at_once():
    d, dn = rm.dumbbell()
    e, n = rm.shifted([(d, dn), (rm.path(9), 9), (rm.clique(5), 5), (rm.dumbbell(70, 3)[0], 143), ([], 2)])
    r, _, c = agree(e, n)
    assert c["components_repaired"] == 3 and c["components"] == 6


# ---- streams ---------------------------------------------------------------------------------------------------------

def stream_graph():
    e, n = rm.planted(260, 4, 0.3, 3, 5)
    return e, n + 1                     # ... and a last vertex without an edge


def test_every_stream_form_gives_the_same_flags():
    e, n = stream_graph()
    base = agree(e, n)
    assert base[0][n - 1] == 1
    rng = np.random.default_rng(3)
    et = dev(e)
    forms = {"stride 1": (et[:, 0].contiguous(), et[:, 1].contiguous()), "flipped": dev(e[:, ::-1]),
             "stride 1 flipped": (et[:, 1].contiguous(), et[:, 0].contiguous())}
    for name, form in forms.items():
        r, re, c = engine.pick_references_dev(form, n)
        assert torch.equal(r.cpu(), torch.as_tensor(base[0])), name
        assert c == base[2], name
        want = base[1][:, ::-1] if "flipped" in name else base[1]
        assert np.array_equal(re.cpu().numpy(), want), name
    twice = np.concatenate([e, e[:, ::-1]])
    shuffled = twice[rng.permutation(len(twice))]
    for name, ee in (("twice", twice), ("shuffled", shuffled)):
        r, re, c = agree(ee, n)
        assert np.array_equal(r, base[0]), name
        assert c["reference_edges"] == 2 * base[2]["reference_edges"]


def test_three_repeats_give_the_same_bits():
    e, n = rm.planted(600, 10, 0.4, 5, 1)
    et = dev(e)
    first = engine.pick_references_dev(et, n)
    for _ in range(2):
        again = engine.pick_references_dev(et, n)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and first[2] == again[2]


def test_no_edges_and_no_vertices():
    r, re, c = agree([], 7)
    assert r.all() and re.shape == (0, 2)
    r, re, c = engine.pick_references_dev(dev(np.zeros((0, 2), dtype=np.int64)), 0)
    assert r.shape == (0,) and re.shape == (0, 2) and all(v == 0 for v in c.values())


# ---- fast mode -------------------------------------------------------------------------------------------------------

def test_fast_mode_component_sizes():
    sizes = (9, 10, 11, 19, 20)
    e, n = rm.shifted([(rm.random_graph(k, 0.3, k), k) for k in sizes])
    r, _, c = agree(e, n, fast=True)
    at = 0
    for k in sizes:
        assert r[at:at + k // 10 + 1].all()
        at += k
    assert c["from_cliques"] == sum(k // 10 + 1 for k in sizes) and c["cliques_removed"] == 0


@pytest.mark.parametrize("m", [2, 3, 4])
def test_fast_mode_merged_counts(m):
    e, n = rm.shifted([(rm.clique(30), 30), (rm.path(12), 12)])
    existing, merged = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    existing[4] = 1
    where = [9, 13, 21, 27][:m]
    merged[where] = 1
    r, _, c = agree(e, n, existing, merged, fast=True)
    assert c["from_small"] == m // 3 + 1 and r[where[:m // 3 + 1]].all()
    assert c["from_cliques"] == 2                   # the path's 12 // 10 + 1; the clique holds an existing reference


def test_fast_mode_component_with_existing_reference_gains_none():
    e, n = rm.shifted([(rm.random_graph(40, 0.5, 2), 40)])
    existing = np.zeros(n, dtype=np.uint8)
    existing[33] = 1
    r, _, c = agree(e, n, existing, fast=True)
    assert np.array_equal(r, existing) and c["references"] == 1


# ---- errors ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("what", ["id == n", "negative", "self-loop"])
def test_first_of_several_bad_edges_is_named_and_a_good_call_follows(where, what):
    e, n = rm.planted(120, 3, 0.3, 2, 9)
    good = e.copy()
    k = {"first": 0, "middle": len(e) // 2, "last": len(e) - 1}[where]
    bad = {"id == n": (3, n), "negative": (-1, 5), "self-loop": (8, 8)}[what]
    e = e.copy()
    e[k] = bad
    if k + 7 < len(e):
        e[k + 7] = (n + 4, 0)                       # a later offender: not the one named
    why = "self-loop" if what == "self-loop" else r"vertex id out of range \[0, %d\)" % n
    with pytest.raises(RuntimeError, match=r"ppk_pick_refs: edge %d \(i=%d, j=%d\): %s" % (k, bad[0], bad[1], why)):
        engine.pick_references_dev(dev(e), n)
    with pytest.raises(RuntimeError, match=r"edge %d \(" % k):
        engine.pick_references(e, n)
    agree(good, n)


def test_scratch_cap_names_the_component_size(ppk_option):
    ppk_option("refs_scratch_mb", 1)
    e = edge_array(rm.path(4000))
    with pytest.raises(RuntimeError, match=r"\(3\): ppk_pick_refs: the largest component has 4000 vertices.*refs_scratch_mb \(1\)"):
        engine.pick_references_dev(dev(e), 4000)
    assert _lib.ERR_CAPACITY == 3
    agree(rm.path(40), 40)                          # a good call after it


def test_option_and_argument_errors(ppk_option):
    e = dev(edge_array(rm.path(5)))
    ppk_option("refs_lds_bits", 63)
    with pytest.raises(RuntimeError, match="refs_lds_bits must be 64 .. 65536"):
        engine.pick_references_dev(e, 5)
    ppk_option("refs_lds_bits", 65536)
    with pytest.raises(TypeError):
        engine.pick_references_dev(e, 5, existing=dev(np.zeros(4, dtype=np.uint8)))
    with pytest.raises(TypeError):
        engine.pick_references_dev(e.to(torch.int32), 5)


def test_host_twin_equals_the_device_call():
    e, n = rm.planted(300, 6, 0.35, 4, 12)
    rng = np.random.default_rng(0)
    existing = (rng.random(n) < 0.03).astype(np.uint8)
    merged = (rng.random(n) < 0.1).astype(np.uint8)
    for fast in (False, True):
        d = on_device(e, n, existing, merged, fast)
        h = engine.pick_references(e, n, existing, merged, fast)
        assert np.array_equal(d[0], h[0]) and np.array_equal(d[1], h[1]) and d[2] == h[2]


# ---- random ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_existing", [False, True])
@pytest.mark.parametrize("p_in,cross", [(0.15, 0), (0.4, 5), (0.7, 5), (0.9, 0)])
def test_planted_graphs(p_in, cross, with_existing):
    e, n = rm.planted(600, 10, p_in, cross, int(p_in * 100))
    existing = None
    if with_existing:
        existing = (np.random.default_rng(7).random(n) < 0.02).astype(np.uint8)
    agree(e, n, existing)
    agree(e, n, existing, fast=True)


# ---- end to end -------------------------------------------------------------------------------------------------------

def partition(numbers):
    """cluster numbers -> every vertex's lowest cluster mate: equal arrays <=> equal partitions"""
    first = {}
    return np.array([first.setdefault(int(c), v) for v, c in enumerate(numbers)], dtype=np.int64)


def test_non_references_assigned_back_give_the_full_partition(tmp_path):
    n = 300
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    tbl = synth.random_match_table(kmers)
    sk, _ = synth.make_sketches(n, kmers, cluster_size=60, seed=3)
    names = ["g%03d" % k for k in range(n)]
    db = engine.SketchDB(np.ascontiguousarray(sk), 16, 14, device=0)
    dist, _ = engine.dist(db, None, kmers, tbl)
    x_max, y_max = synth.boundary_for_quantile(dist.cpu().numpy(), 0.12)
    model = models.RefineBoundary(scale=(1.0, 1.0), slope=2, optimal_x=x_max, optimal_y=y_max)
    edges, _ = model.edges_from_sketches(db, None, kmers, tbl)
    db.close()
    out = tmp_path / "refs"
    out.mkdir()
    idx, ref_names, ref_file, G_ref = network.extractReferences((edges, n), names, str(out))
    assert 0 < len(idx) < n and ref_names == [names[k] for k in idx]
    assert open(ref_file).read() == "".join(s + "\n" for s in ref_names)
    e_host = edges.cpu().numpy()
    flags = np.zeros(n, dtype=np.uint8)
    flags[idx] = 1
    assert rm.check_properties(e_host, n, flags, G_ref[0].cpu().numpy()) == []

    rest = np.setdiff1d(np.arange(n), idx)
    ref_db = engine.SketchDB(np.ascontiguousarray(sk[idx]), 16, 14, device=0)
    qry_db = engine.SketchDB(np.ascontiguousarray(sk[rest]), 16, 14, device=0)
    q_edges, _ = model.edges_from_sketches(ref_db, qry_db, kmers, tbl)
    ref_db.close()
    qry_db.close()
    numbers, _ = engine.cluster_extend_dev(q_edges, assign.component_labels(G_ref), len(rest))
    back = np.empty(n, dtype=np.int64)
    back[np.concatenate([idx, rest])] = numbers.cpu().numpy()
    full, _ = engine.cluster_numbers_dev(edges, n)
    assert np.array_equal(partition(back), partition(full.cpu().numpy()))
    assert len(set(full.cpu().tolist())) > 1
