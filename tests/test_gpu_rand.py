"""GPU tests of the contingency sums (ppk_contingency_sums*, engine.contingency_sums_dev, poppunk_amd.scores' Rand
indices, poppunk_amd.rand_indices): all six outputs against the numpy restatement
(tests/contingency_model.py) with array_equal -- they are integers -- at every size where the routing changes; every
routing option against the default routing; the first-offender error by message; the Python scores against the floats
recorded from sklearn 1.7.2 and the reference script with ==."""
import ctypes as C
import os

import numpy as np
import pytest

import contingency_model as model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poppunk_amd import _lib, engine, rand_indices, scores  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
WAVE = 64          # rand_wave_max's default: the longest class the wave route takes
TABLE = 8192       # the ranks one LDS table holds
SIZES = [1, 2, 3, WAVE - 1, WAVE, WAVE + 1, 257]      # n is also the length of the all-in-one class


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV)


def labelings(n, seed=0):
    """The issue's labelings of n samples, numbers in [1, n]: {name: int32 [n]}."""
    rng = np.random.default_rng(31 * n + seed)
    out = {"one": np.ones(n), "identity": np.arange(1, n + 1), "permuted": rng.permutation(n) + 1}
    two = rng.integers(1, 3, n)
    two[0], two[-1] = 1, min(2, n)
    out["two"] = two
    giant = np.full(n, n)                                   # one giant cluster, numbered n, and singletons
    k = n // 4
    giant[rng.permutation(n)[:k]] = np.arange(1, k + 1)
    out["giant"] = giant
    values = np.array([1, 5, n] if n >= 5 else [1, n])
    gaps = values[rng.integers(0, len(values), n)]
    gaps[0], gaps[-1] = 1, n
    out["gaps"] = gaps
    coarse = rng.integers(1, 5, n)                          # a nested pair: fine refines coarse
    out["coarse"] = np.minimum(coarse, n)
    out["fine"] = np.minimum(3 * coarse - rng.integers(0, 3, n), n) if n >= 12 else out["coarse"].copy()
    k = min(n, int(np.sqrt(n)) + 2)                         # two independent labelings, k * k > n
    out["random_a"], out["random_b"] = rng.integers(1, k + 1, n), rng.integers(1, k + 1, n)
    return {name: v.astype(np.int32) for name, v in out.items()}


def run(levels_a, levels_b=None):
    got = engine.contingency_sums_dev(dev(np.atleast_2d(levels_a)), None if levels_b is None else
                                      dev(np.atleast_2d(levels_b)))
    return tuple(t.cpu().numpy() for t in got)


def assert_same(got, want, what=""):
    names = ("sq_a", "sq_b", "labels_a", "labels_b", "sq_cells", "n_cells")
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_labelings_against_the_model(n):
    lab = labelings(n)
    levels = np.stack(list(lab.values()))
    want = model.contingency_sums(levels)
    got = run(levels)
    assert_same(got, want, "every level against every level")
    # B = NULL against an explicit B = A, and a rectangle
    assert_same(run(levels, levels), want, "explicit B = A")
    assert_same(run(levels[:3], levels[3:]), model.contingency_sums(levels[:3], levels[3:]), "3 x 7")
    assert_same(run(levels[4], levels[7:]), model.contingency_sums(levels[4], levels[7:]), "1 x 3")
    if n >= 12:
        names = list(lab)
        fine, coarse = names.index("fine"), names.index("coarse")
        refines = got[5] == got[2].astype(np.int64)[:, None]
        assert refines[fine, coarse] and not refines[coarse, fine]
        assert got[2][names.index("random_a")] * got[2][names.index("random_b")] > n


@pytest.mark.parametrize("k", [TABLE - 1, TABLE, TABLE + 1])
def test_rank_tables_at_and_around_one_window(k):
    """Both levels have k labels: k - 1 singletons and one class of 300, which takes the table route over the other
    level's k ranks -- one window up to 8 192, two beyond."""
    n = k - 1 + 300
    rng = np.random.default_rng(k)
    levels = []
    for _ in range(2):
        level = np.empty(n, dtype=np.int32)
        where = rng.permutation(n)
        level[where[:300]] = k + 7                          # (a number with a gap before it)
        level[where[300:]] = rng.permutation(k - 1) + 1
        levels.append(level)
    levels = np.stack(levels + [labelings(n)["random_a"]])
    got = run(levels)
    assert got[2].tolist()[:2] == [k, k]
    assert_same(got, model.contingency_sums(levels), "k = %d" % k)


@pytest.fixture(scope="module")
def routed():
    """The default routing's results, computed once: n = 257 with every labeling; n = 8 500 with two levels of 8 193
    labels (two rank windows) and two random ones; n = 3 000 with 16 x 16 levels (1.1 MB of per-level state)."""
    out = {}
    out[257] = (np.stack(list(labelings(257).values())), None)
    n = 8500
    rng = np.random.default_rng(9)
    wide = []
    for _ in range(2):
        level = np.empty(n, dtype=np.int32)
        where = rng.permutation(n)
        level[where[:n - 8192]] = n
        level[where[n - 8192:]] = rng.permutation(8192) + 1
        wide.append(level)
    lab = labelings(n)
    out[8500] = (np.stack(wide + [lab["random_a"], lab["giant"]]), None)
    rng = np.random.default_rng(10)
    out[3000] = (np.stack([rng.integers(1, 2 + 40 * t, 3000) for t in range(16)]).astype(np.int32),
                 np.stack([rng.integers(1, 3000 - 150 * t, 3000) for t in range(16)]).astype(np.int32))
    return {n: (a, b, run(a, b)) for n, (a, b) in out.items()}


def test_default_routing_of_the_routed_shapes_against_the_model(routed):
    for n in (8500, 3000):
        a, b, got = routed[n]
        assert_same(got, model.contingency_sums(a, b), "n = %d" % n)
    assert routed[8500][2][2].tolist()[:2] == [8193, 8193]


FORCE_WAVE = (1 << 31) - 1


@pytest.mark.parametrize("option,value,n", [("rand_wave_max", 0, 257), ("rand_wave_max", 1, 257),
                                            ("rand_wave_max", FORCE_WAVE, 257), ("rand_wave_max", 100, 257),
                                            ("rand_window", 8, 257), ("rand_window", 1, 257),
                                            ("rand_wave_max", 0, 8500), ("rand_wave_max", FORCE_WAVE, 8500),
                                            ("rand_window", -1, 8500), ("rand_window", 1000, 8500),
                                            ("rand_batch", 1, 257), ("rand_batch", 7, 257), ("rand_batch", 7, 3000),
                                            ("rand_scratch_mb", 1, 3000)])
def test_every_routing_gives_the_integers_of_the_default(routed, ppk_option, option, value, n):
    a, b, want = routed[n]
    ppk_option(option, value)
    assert_same(run(a, b), want, "%s = %d" % (option, value))


def test_both_routes_forbidden_windows_and_forced_windows_together(routed, ppk_option):
    a, b, want = routed[8500]
    ppk_option("rand_wave_max", 0)
    ppk_option("rand_window", 64)
    assert_same(run(a, b), want, "every class through windows of 64 ranks")


def test_sums_and_keys_past_2_to_the_32():
    """n = 70 000: all-in-one has sum = 4.9e9; a permuted singleton level against a 300-label level makes a key
    x * K_y + y pass 2^32.  32-bit accumulators or keys fail here."""
    n = 70000
    rng = np.random.default_rng(70)
    levels = np.stack([np.ones(n), rng.permutation(n) + 1, (rng.integers(0, 300, n) * 233 + 1)]).astype(np.int32)
    got = run(levels)
    assert got[0][0] == n * n > 1 << 32 and got[4][0, 0] == n * n
    assert n * (n + 1) > 1 << 32                            # (the restatement's own keys are int64)
    assert_same(got, model.contingency_sums(levels), "n = 70 000")
    assert_same(run(levels[:2], levels[1:]), model.contingency_sums(levels[:2], levels[1:]), "2 x 2")
    # all-in-one against itself as an explicit pair: one class of 70 000 through the table route
    assert_same(run(levels[:1], levels[:1]), model.contingency_sums(levels[:1], levels[:1]), "1 x 1")


def test_first_offender_error_names_side_level_sample_and_value():
    n = 65
    lab = labelings(n)
    a = np.stack([lab["two"], lab["giant"], lab["random_a"]])
    b = np.stack([lab["fine"], lab["coarse"]])
    for value in (0, n + 1):
        bad = a.copy()
        bad[-1, -1] = value
        for args in ((bad, None), (bad, b)):
            with pytest.raises(RuntimeError) as e:
                run(*args)
            assert "ppk_contingency_sums: side a, level 2, sample %d: label %d outside [1, %d]" % (n - 1, value, n) \
                in str(e.value)
        bad_b = b.copy()
        bad_b[-1, -1] = value
        with pytest.raises(RuntimeError) as e:
            run(a, bad_b)
        assert "ppk_contingency_sums: side b, level 1, sample %d: label %d outside [1, %d]" % (n - 1, value, n) \
            in str(e.value)
    # the first of several: A's levels come before B's
    bad, bad_b = a.copy(), b.copy()
    bad[1, 7], bad[2, 3], bad_b[0, 0] = -4, 0, 0
    with pytest.raises(RuntimeError) as e:
        run(bad, bad_b)
    assert "side a, level 1, sample 7: label -4 outside [1, 65]" in str(e.value)
    # the call after a refused one is unaffected
    assert_same(run(a, b), model.contingency_sums(a, b))


def test_host_form_equals_the_device_form(routed):
    for n in (257, 3000):
        a, b, want = routed[n]
        got = scores._device_sums(a, b)
        assert_same(got, want, "host form, n = %d" % n)
    # ... without the outputs of B where B = A
    a = np.ascontiguousarray(routed[257][0], dtype=np.int32)
    n_a, n = a.shape
    sq_a, labels_a = np.empty(n_a, dtype=np.int64), np.empty(n_a, dtype=np.int32)
    sq_cells, n_cells = np.empty((n_a, n_a), dtype=np.int64), np.empty((n_a, n_a), dtype=np.int64)
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    _lib.check(_lib.lib().ppk_contingency_sums(a.ctypes.data_as(ip), n_a, None, 0, n, 0, sq_a.ctypes.data_as(lp), None,
                                               labels_a.ctypes.data_as(ip), None, sq_cells.ctypes.data_as(lp),
                                               n_cells.ctypes.data_as(lp)), "ppk_contingency_sums")
    want = routed[257][2]
    assert np.array_equal(sq_a, want[0]) and np.array_equal(labels_a, want[2])
    assert np.array_equal(sq_cells, want[4]) and np.array_equal(n_cells, want[5])


def test_python_scores_equal_the_recorded_floats():
    z = np.load(os.path.join(HERE, "golden", "rand.npz"))
    for k in range(int(z["n_pairs"])):
        t, p = z["pair%d_true" % k], z["pair%d_pred" % k]
        assert np.array_equal(scores.pair_confusion_matrix(t, p), z["pair%d_confusion" % k]), k
        assert scores.rand_score(t, p) == float(z["pair%d_rand" % k]), k
        assert scores.adjusted_rand_score(t, p) == float(z["pair%d_ari" % k]), k
        assert scores.rand_index_score(t, p) == float(z["pair%d_ri" % k]), k
    # one device call for a family, on resident levels
    fine, coarse = scores.factorise(z["pair6_true"])[0], scores.factorise(z["pair6_pred"])[0]
    rand, adjusted, refines = scores.rand_of_levels(dev(np.stack([fine, coarse])))
    assert rand[0, 1] == rand[1, 0] == float(z["pair6_rand"])
    assert adjusted[0, 1] == adjusted[1, 0] == float(z["pair6_ari"])
    assert refines.tolist() == [[True, True], [False, True]]
    rand, adjusted, refines = scores.rand_of_levels(dev(fine[None, :]), dev(coarse[None, :]))
    assert rand[0, 0] == float(z["pair6_rand"]) and adjusted[0, 0] == float(z["pair6_ari"]) and refines[0, 0]


@pytest.mark.parametrize("run_name", ["same_names_subset", "lacking_names"])
def test_calculate_rand_indices_writes_the_script_s_bytes(tmp_path, monkeypatch, capsys, run_name):
    z = np.load(os.path.join(HERE, "golden", "rand.npz"))
    for name, text in zip(z["file_names"], z["file_texts"]):
        (tmp_path / str(name)).write_text(str(text))
    monkeypatch.chdir(tmp_path)
    rand_indices.calculate_rand_indices([str(a) for a in z[run_name + "_args"]], output="mine.out",
                                        subset=str(z[run_name + "_subset"]) or None)
    assert open("mine.out").read() == str(z[run_name + "_out"])
    assert capsys.readouterr().err == str(z[run_name + "_err"])
