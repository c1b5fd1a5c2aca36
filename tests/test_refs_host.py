"""CPU tests of reference picking's host side: the numpy restatement of the rule on hand cases whose
answer is worked out here, P1-P3 by the independent checker on 20 planted graphs, every claim a graph builder makes,
writeReferences' bytes, extractReferences' argument handling (the engine call replaced by the restatement), the
command line's parser, and the reference's own picks (tests/golden/references.npz): they satisfy the same properties,
and our .refs file for the same names has the same bytes."""
import os
import re

import numpy as np
import pytest

import refs_model as rm
from poppunk_amd import _lib, network, reference_pick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def refs_of(e, n, **kw):
    r, re_, c = rm.pick_refs(e, n, **kw)
    assert rm.check_properties(e, n, r, re_, clique_mode=not kw.get("fast", False)) == []
    return np.flatnonzero(r).tolist(), re_.tolist(), c


# ---- the restatement on hand cases -----------------------------------------------------------------------------------

def test_hand_cases():
    assert refs_of(rm.clique(3), 3)[0] == [0]
    # path 0-1-2: {0, 1} gives 0, the leftover {2} gives 2, the repair adds 1 between them
    idx, re_, c = refs_of(rm.path(3), 3)
    assert idx == [0, 1, 2] and re_ == [[0, 1], [1, 2]] and c["added_by_repair"] == 1 and c["cliques_removed"] == 2
    # components of one and two vertices: the lowest vertex, even beside an existing reference
    idx, _, c = refs_of([(0, 1), (3, 4)], 5, existing=[0, 1, 0, 0, 1])
    assert idx == [0, 1, 2, 3, 4] and c["from_small"] == 3 and c["references"] == 5
    # a square with one diagonal, 0-1-2-3-0 and 0-2: K = {0, 1, 2}, then {3}: 3 is next to 0, no repair
    idx, re_, c = refs_of([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)], 4)
    assert idx == [0, 3] and re_ == [[1, 0]] and c["components_repaired"] == 0
    # orientation and order of the reference edges are the stream's; a repeated edge comes out twice
    idx, re_, _ = refs_of([(3, 0), (0, 3), (2, 3), (1, 2), (0, 1), (2, 0)], 4)
    assert idx == [0, 3] and re_ == [[1, 0], [0, 1]]
    # an existing reference anywhere in the clique suppresses the pick
    idx, _, c = refs_of(rm.clique(6), 6, existing=[0, 0, 0, 0, 1, 0])
    assert idx == [4] and c["from_cliques"] == 0
    assert refs_of(rm.clique(200), 200)[0] == [0]
    assert refs_of([], 300)[0] == list(range(300))


def test_hand_cases_fast_mode():
    # 11 vertices: 11 // 10 + 1 = 2 lowest; 9 vertices: 1
    e, n = rm.shifted([(rm.path(11), 11), (rm.path(9), 9)])
    idx, _, c = refs_of(e, n, fast=True)
    assert idx == [0, 1, 11] and c["from_cliques"] == 3 and c["cliques_removed"] == 0
    # an existing reference: none gained; 4 merged queries in it: the 4 // 3 + 1 = 2 lowest, joined to it by the repair
    existing, merged = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    existing[5] = 1
    merged[[2, 3, 7, 9]] = 1
    idx, _, c = refs_of(e, n, existing=existing, merged=merged, fast=True)
    assert idx == [2, 3, 4, 5, 11] and c["from_small"] == 2 and c["added_by_repair"] == 1


def test_bad_edges_are_refused():
    for e in ([(0, 3)], [(-1, 0)], [(1, 1)]):
        with pytest.raises(ValueError):
            rm.pick_refs(e, 3)


# ---- properties ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(20))
def test_properties_on_planted_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(120, 320))
    e, n = rm.planted(n, int(rng.integers(2, 9)), float(rng.uniform(0.1, 0.9)), int(rng.integers(0, 6)), seed)
    existing = (rng.random(n) < 0.03).astype(np.uint8) if seed % 2 else None
    r, re_, c = rm.pick_refs(e, n, existing)
    assert rm.check_properties(e, n, r, re_) == []
    assert c["references"] == int(r.sum()) and c["reference_edges"] == len(re_)
    shuffled = e[rng.permutation(len(e))][:, ::-1]
    assert np.array_equal(rm.pick_refs(shuffled, n, existing)[0], r)       # the order of the edges does not matter
    r, re_, _ = rm.pick_refs(e, n, existing, fast=True)
    assert rm.check_properties(e, n, r, re_, clique_mode=False) == []


def test_the_checker_finds_violations():
    e, n = rm.dumbbell()
    r, re_, _ = rm.pick_refs(e, n)
    assert rm.check_properties(e, n, r, re_) == []
    broken = r.copy()
    broken[np.flatnonzero(r)[1]] = 0                 # a bridge vertex: the two ends fall apart
    assert any(m.startswith("P2") for m in rm.check_properties(e, n, broken))
    none = np.zeros(n, dtype=np.uint8)
    assert any(m.startswith("P1") for m in rm.check_properties(e, n, none))
    assert any("not the stream's" in m for m in rm.check_properties(e, n, r, re_[::-1]))


# ---- the builders' claims --------------------------------------------------------------------------------------------

def components_of(e, n):
    lab = rm._sets([tuple(x) for x in np.asarray(e).reshape(-1, 2).tolist()], n)
    sizes = {}
    for v in range(n):
        sizes[lab[v]] = sizes.get(lab[v], 0) + 1
    return sorted(sizes.values())


def test_builders():
    assert len(rm.clique(65)) == 65 * 64 // 2 and components_of(rm.clique(65), 65) == [65]
    assert len(rm.path(129)) == 128 and components_of(rm.path(129), 129) == [129]
    for lowest in (True, False):
        s = rm.star(100, lowest)
        assert len(s) == 100 and components_of(s, 101) == [101]
        assert all((0 if lowest else 100) in edge for edge in s)
    for k in (2, 3, 63, 64, 65, 127, 128, 129):
        g = rm.random_graph(k, 0.5, 100 + k)
        assert components_of(g, k) == [k] and len(set(g)) == len(g) and all(a < b for a, b in g)
    e, n = rm.dumbbell()
    assert n == 46 and components_of(e, n) == [46]
    assert rm.pick_refs(e, n)[2]["components_repaired"] == 1            # "this dumbbell needs repair"
    e, n, existing = rm.far_existing(5)
    assert n == 6 and np.flatnonzero(existing).tolist() == [0, 5]
    r, _, c = rm.pick_refs(e, n, existing)
    assert r.all() and c["components_repaired"] == 1
    e, n = rm.planted(600, 10, 0.4, 0, 1)
    assert n == 600 and len(components_of(e, n)) >= 10 and max(components_of(e, n)) <= 60
    e, n = rm.shifted([(rm.path(3), 3), ([], 2), (rm.clique(4), 4)])
    assert n == 9 and components_of(e, n) == [1, 1, 3, 4] and e.min() == 0 and e.max() == 8


# ---- writeReferences, extractReferences ------------------------------------------------------------------------------

def test_write_references_bytes(tmp_path):
    out = tmp_path / "db"
    out.mkdir()
    name = network.writeReferences(["b/x.fa", "a", "c d"], str(out), outSuffix=".new")
    assert name == str(out) + "/db.new.refs"
    assert open(name, "rb").read() == b"b/x.fa\na\nc d\n"
    assert open(network.writeReferences([], str(out)), "rb").read() == b""


def test_extract_references_argument_handling(tmp_path, monkeypatch, capsys):
    seen = {}

    def restated(edges, n, existing, merged, fast):
        seen.update(existing=existing, merged=merged, fast=fast)
        return rm.pick_refs(edges, n, existing, merged, fast)
    monkeypatch.setattr(network, "_pick_references", restated)
    e, n = rm.dumbbell()
    names = ["g%02d" % (n - 1 - k) for k in range(n)]                       # not in sorted order
    out = tmp_path / "picked"
    out.mkdir()
    idx, ref_names, ref_file, G_ref = network.extractReferences((np.asarray(e), n), names, str(out))
    err = capsys.readouterr().err
    assert err == "Running clique finding\nReconstructing clusters with shortest paths\n"
    assert isinstance(idx, np.ndarray) and idx.dtype == np.int64 and np.all(np.diff(idx) > 0)
    assert ref_names == [names[k] for k in idx] and ref_file == str(out) + "/picked.refs"
    assert open(ref_file).read() == "".join(s + "\n" for s in ref_names)
    assert G_ref[1] == len(idx) and np.asarray(G_ref[0]).max() < len(idx)
    assert seen == {"existing": None, "merged": None, "fast": False}

    # positional order of the reference: G, dbOrder, outPrefix, merged_queries, outSuffix, existingRefs, threads,
    # use_gpu, fast_mode
    idx2, _, ref_file2, _ = network.extractReferences((np.asarray(e), n), names, str(out), [names[3], names[3]], ".v2",
                                                      [names[7]], 4, True, True)
    assert capsys.readouterr().err.startswith("Running quick reference picking\n")
    assert ref_file2.endswith("/picked.v2.refs") and seen["fast"] is True
    assert np.flatnonzero(seen["existing"]).tolist() == [7] and np.flatnonzero(seen["merged"]).tolist() == [3]
    assert 7 in idx2 and 3 in idx2
    with pytest.raises(KeyError):
        network.extractReferences((np.asarray(e), n), names, str(out), existingRefs=["nobody"])
    with pytest.raises(ValueError):
        network.extractReferences((np.asarray(e), n), names[:-1], str(out))


# ---- the command line ------------------------------------------------------------------------------------------------

def test_cli_parser(tmp_path):
    p = reference_pick.get_parser()
    a = p.parse_args(["--network", "n.npz", "--distances", "d", "--output", "o"])
    assert (a.network, a.distances, a.output, a.ref_db, a.model, a.clusters, a.threads, a.use_gpu) == \
        ("n.npz", "d", "o", None, None, None, 1, False)
    a = p.parse_args(["--network", "n.npz", "--distances", "d", "--output", "o", "--ref-db", "db", "--model", "m",
                      "--clusters", "c.csv", "--threads", "8", "--use-gpu"])
    assert (a.ref_db, a.model, a.clusters, a.threads, a.use_gpu) == ("db", "m", "c.csv", 8, True)
    for missing in ("--network", "--distances", "--output"):
        args = [x for pair in (("--network", "n"), ("--distances", "d"), ("--output", "o")) if pair[0] != missing
                for x in pair]
        with pytest.raises(SystemExit):
            p.parse_args(args)
    text = re.sub(r"\s+", " ", p.format_help())
    assert ".npz" in text and "graph-tool and cugraph files cannot be read" in text and p.prog == "poppunk_references"
    G = (np.array([[0, 2], [2, 1]]), 4)
    os.makedirs(tmp_path / "x")
    name = reference_pick.save_network_npz(G, str(tmp_path / "x"), ".refs_graph")
    assert name.endswith("/x/x.refs_graph.npz")
    edges, n = reference_pick.load_network_npz(name)
    assert n == 4 and edges.tolist() == [[0, 2], [2, 1]] and edges.dtype == np.int64


def test_symbols_and_options_are_declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppk.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name, n_args in (("ppk_pick_refs_dev", 12), ("ppk_pick_refs", 11)):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args
    for name, default in (("refs_scratch_mb", 4096), ("refs_lds_bits", 65536)):
        if "PPK_" + name.upper() not in os.environ:
            assert _lib.get_option(name) == default
    assert "ppk_refs.hip" in open(os.path.join(ROOT, "poppunk_amd", "csrc", "Makefile")).read()


# ---- the reference's own picks ---------------------------------------------------------------------------------------

def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "references.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("k", range(7))
def test_the_references_own_choice_has_the_properties(k, tmp_path):
    g = golden()
    assert int(g["cases"]) == 7
    n, e, fast = int(g["n_%d" % k]), g["edges_%d" % k], bool(g["fast_%d" % k])
    chosen, existing = g["chosen_%d" % k], g["existing_%d" % k]
    assert n <= 300 and set(np.flatnonzero(existing).tolist()) <= set(chosen.tolist())
    flags = np.zeros(n, dtype=np.uint8)
    flags[chosen] = 1
    # P1-P3 are the reference's contract, not ours alone (P1 over its own clique order: domination)
    assert rm.check_properties(e, n, flags, None, clique_mode=not fast, own_cliques=False) == []
    ours, re_, c = rm.pick_refs(e, n, existing if existing.any() else None, None, fast)
    assert rm.check_properties(e, n, ours, re_, clique_mode=not fast) == []
    print("case %d: the stand-in's loop picked %d references, the rule %d" % (k, len(chosen), c["references"]))
    out = tmp_path / "db"
    out.mkdir()
    names = ["s%03d" % v for v in range(n)]
    ref_file = network.writeReferences([names[v] for v in chosen], str(out))
    assert open(ref_file, "rb").read() == g["refs_file_%d" % k].tobytes()
