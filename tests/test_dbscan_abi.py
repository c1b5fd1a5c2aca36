"""CPU tests of the DBSCAN section of the C ABI: every ppk_dbscan_* symbol include/ppk.h declares is exported and
bound, and argument errors come back as status codes with a message, before any device is touched."""
import ctypes as C
import os
import re

import numpy as np

from poppunk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ppk_dbscan_core_dev", "ppk_dbscan_mst_dev", "ppk_dbscan_fit", "ppk_dbscan_create", "ppk_dbscan_destroy",
         "ppk_dbscan_assign_dev", "ppk_dbscan_edges_dev", "ppk_dbscan_assign", "ppk_dbscan_stats")


def test_dbscan_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ppk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ppk_dbscan_[a-z0-9_]+)\s*\(", src))
    assert declared == set(NAMES)
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "ppk_dbscan.hip" in open(os.path.join(ROOT, "poppunk_amd", "csrc", "Makefile")).read()
    assert _lib.sources_hash_now() == _lib.source_hash()        # the new file is part of the build's hash


def test_the_unverified_steps_are_marked_in_the_header():
    src = open(os.path.join(ROOT, "include", "ppk.h")).read()
    section = src[src.index("DBSCAN: fitting and assigning"):src.index("int ppk_dbscan_core_dev")]
    for step in ("1. [EXT]", "2. [EXT]", "3. [EXT]", "4. [EXT]", "5. [EXT]"):
        assert step in section


def test_argument_errors_are_status_codes():
    lib = _lib.lib()
    pts = np.zeros((4, 2), dtype=np.float32)
    out = np.zeros(4)
    p, o = C.c_void_p(pts.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.ppk_dbscan_core_dev(p, 4, 0, o, None) == _lib.ERR_ARG and "min_samples" in _lib.last_error()
    assert lib.ppk_dbscan_core_dev(p, 4, 4, o, None) == _lib.ERR_ARG and "needs at least 5 points" in _lib.last_error()
    assert lib.ppk_dbscan_core_dev(p, 1 << 31, 3, o, None) == _lib.ERR_ARG and "2^31" in _lib.last_error()
    assert lib.ppk_dbscan_core_dev(None, 4, 1, o, None) == _lib.ERR_ARG
    assert lib.ppk_dbscan_mst_dev(p, o, 1 << 31, o, o, o, None) == _lib.ERR_ARG
    assert lib.ppk_dbscan_mst_dev(p, o, 0, o, o, o, None) == _lib.ERR_ARG

    f32p, f64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    core2, lam, birth = np.zeros(4), np.ones(4), np.zeros(1)
    cluster, parent, label = np.zeros(4, dtype=np.int32), np.array([-1], dtype=np.int32), np.array([-1], dtype=np.int32)

    def create(n=4, m=2, scale=(1.0, 1.0), parent=parent, cluster=cluster, n_cl=1):
        s = np.asarray(scale, dtype=np.float64)
        h = C.c_void_p()
        rc = lib.ppk_dbscan_create(pts.ctypes.data_as(f32p), core2.ctypes.data_as(f64p), n, m,
                                   cluster.ctypes.data_as(i32p), lam.ctypes.data_as(f64p), parent.ctypes.data_as(i32p),
                                   birth.ctypes.data_as(f64p), label.ctypes.data_as(i32p), n_cl, s.ctypes.data_as(f64p),
                                   0, 0, 0, C.byref(h))
        assert h.value is None or rc == _lib.OK
        return rc
    assert create(m=0) == _lib.ERR_ARG and "min_samples" in _lib.last_error()
    assert create(scale=(1.0, 0.0)) == _lib.ERR_ARG and "scale" in _lib.last_error()
    assert create(scale=(-1.0, 1.0)) == _lib.ERR_ARG
    assert create(n=1 << 31) == _lib.ERR_ARG and "2^31" in _lib.last_error()
    assert create(parent=np.array([0], dtype=np.int32)) == _lib.ERR_ARG and "root" in _lib.last_error()
    assert create(cluster=np.array([0, 0, 3, 0], dtype=np.int32)) == _lib.ERR_ARG and "point 2" in _lib.last_error()
    # a NULL handle
    lab = np.zeros(4, dtype=np.int32)
    assert lib.ppk_dbscan_assign(pts.ctypes.data_as(f32p), 4, None, lab.ctypes.data_as(i32p)) == _lib.ERR_ARG
    assert lib.ppk_dbscan_assign_dev(p, 4, None, o, None) == _lib.ERR_ARG
    assert lib.ppk_dbscan_edges_dev(p, 4, 0, None, 0, o, 4, o, None) == _lib.ERR_ARG
    lib.ppk_dbscan_destroy(None)
