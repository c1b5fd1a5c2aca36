#!/usr/bin/env python
"""Generates tests/golden/sketch_qc.json from the reference checkout: PopPUNK.qc.sketchlibAssemblyQC
(PopPUNK/qc.py:137-236) run, unchanged, on small databases.

Run in the BUILD container only (needs /root/reference); the fixture is data (inputs + the reference's answers) and is
committed, the reference is not.  The function body is taken from the reference file by name (as make_golden.py does)
and executed as it is.  It opens `<prefix>/<basename>.h5` with h5py, which this container does not have, and then only
indexes the file object, iterates its 'sketches' group and reads `.attrs`: a stand-in `h5py.File` made of dicts answers
exactly those three, so every line that decides the result is the reference's own.
"""
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, extract_functions  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


class Node(dict):
    """a group: a dict of children with an `attrs` dict"""

    def __init__(self, children=(), attrs=None):
        super().__init__(children)
        self.attrs = dict(attrs or {})


DATABASES = {}


class File(Node):
    def __init__(self, path, mode="r"):
        super().__init__({"sketches": DATABASES[path]})

    def close(self):
        pass


def database(samples):
    """{name: (length, missing_bases, reads or None)} -> the stand-in's /sketches group"""
    grp = Node()
    for name, (length, missing, reads) in samples.items():
        attrs = {"length": length, "missing_bases": missing}
        if reads is not None:
            attrs["reads"] = reads
        grp[name] = Node(attrs=attrs)
    return grp


def main():
    h5py = types.ModuleType("h5py")
    h5py.File = File
    sys.modules["h5py"] = h5py
    pkg = types.ModuleType("refpkg")
    pkg.__path__ = []
    sub = types.ModuleType("refpkg.sketchlib")
    sub.removeFromDB = lambda *a, **k: None
    sys.modules["refpkg"], sys.modules["refpkg.sketchlib"] = pkg, sub
    ns = {"np": np, "os": os, "sys": sys, "__package__": "refpkg", "__name__": "refpkg.qc"}
    extract_functions(os.path.join(REF, "PopPUNK", "qc.py"), ["sketchlibAssemblyQC"], ns)
    run = ns["sketchlibAssemblyQC"]

    rng = np.random.Generator(np.random.PCG64(20261020))
    lengths = [int(x) for x in rng.normal(2_000_000, 20_000, size=12)]
    base = {"s%02d" % i: (lengths[i], int(rng.integers(0, 50)), None) for i in range(12)}
    short_long = dict(base, s03=(1_200_000, 10, None), s07=(2_900_000, 10, None))
    many_n = dict(base, s02=(lengths[2], 5_000, None), s05=(lengths[5], 250_000, None))
    both = dict(base, s04=(900_000, 400_000, None), s09=(lengths[9], 300_000, None))
    reads = dict(base, s01=(lengths[1], 900_000, True), s06=(lengths[6], 900_000, False), s08=(lengths[8], 900_000, None))
    default_qc = {"upper_n": None, "prop_n": 0.1, "length_sigma": 5, "length_range": [None, None]}
    cases = [
        ("length cut-off by sigma", short_long, dict(default_qc, length_sigma=2), None),
        ("length cut-off by range", short_long, dict(default_qc, length_range=[1_500_000, 2_500_000]), None),
        ("ambiguous bases by proportion", many_n, dict(default_qc, prop_n=0.05), None),
        ("ambiguous bases by count", many_n, dict(default_qc, upper_n=1_000), None),
        ("a sample failing both", both, dict(default_qc, length_sigma=2), None),
        ("the reads attribute", reads, dict(default_qc, prop_n=0.1), None),
        ("a subset of the names, in another order", short_long, dict(default_qc, length_sigma=2),
         ["s07", "s00", "s03", "s11", "not_in_db"]),
    ]
    out = {"source": "PopPUNK/qc.py:137-236 sketchlibAssemblyQC run by tests/golden/make_golden_sketch_qc.py over a "
                     "stand-in for the h5py file object", "cases": []}
    for what, samples, qc, names in cases:
        prefix = "/db/%d" % len(out["cases"])
        DATABASES[prefix + "/" + os.path.basename(prefix) + ".h5"] = database(samples)
        names = sorted(samples) if names is None else names
        retained, failed = run(prefix, names, qc)
        out["cases"].append({"what": what, "samples": {k: list(v) for k, v in samples.items()}, "qc_dict": qc,
                             "names": names, "retained": retained, "failed": failed})
    with open(os.path.join(HERE, "sketch_qc.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("sketch_qc.json:", len(out["cases"]), "cases;",
          [len(c["failed"]) for c in out["cases"]], "failures each")


if __name__ == "__main__":
    main()
