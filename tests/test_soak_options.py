"""tests/soak_case.py sets run-time options case after case; reset_options() must leave every one of them, and the
options other suites' cases may have left set, at the library's default."""
import inspect
import re

import soak_case
from poppunk_amd import _lib

# the options of the coded copies and five more that reset_options() once left as a case (or another suite's) set them,
# with PpkConfig's defaults
LATE = {"rank_planes": 1, "rank_short": 1, "rank_fold": 1, "rank_fold2": 1, "sweep_window": 1, "knn_lane_lists": 0,
        "ksplit_scratch_mb": 2048, "pairs_chunk": 0, "pairs_scratch_mb": 1024}


def test_reset_options_restores_every_option_a_case_sets():
    names = set(re.findall(r'set_option\("(\w+)"', inspect.getsource(soak_case.soak_case))) | set(LATE)
    assert {"rank_planes", "rank_short", "rank_fold", "rank_fold2", "ksplit", "db_cache"} <= names
    defaults = {name: _lib.get_option(name) for name in names}
    assert {name: defaults[name] for name in LATE} == LATE
    try:
        for name in names:
            _lib.set_option(name, defaults[name] + 1)
        assert all(_lib.get_option(name) == defaults[name] + 1 for name in names)
        soak_case.reset_options()
        assert {name: _lib.get_option(name) for name in names} == defaults
    finally:
        for name, value in defaults.items():
            _lib.set_option(name, value)
