"""ppk_sweep_boundaries_1d: the boundaries of a 1-D sweep, the one statement of them (no device is touched).

The reference is a numpy restatement of thresholdIterate1D's arithmetic (src/boundary.cpp:161-186) with its float /
double mix kept: float differences, a float square root and quotients, the offset multiplied in double and rounded to
float, the slope-2 intercepts in float.  Equality is on the bits."""
import ctypes as C

import numpy as np
import pytest

from poppunk_amd import _lib, engine

f32 = np.float32


def _restated(offsets, slope, x0, y0, x1, y1):
    x0, y0, x1, y1 = f32(x0), f32(y0), f32(x1), f32(y1)
    dx, dy = f32(x1 - x0), f32(y1 - y0)
    ds = np.sqrt(f32(f32(dx * dx) + f32(dy * dy)), dtype=f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        gradient = f32(dy / dx)
        ux, uy = np.float64(f32(dx / ds)), np.float64(f32(dy / ds))
        off = np.asarray(offsets, dtype=np.float64)
        x_int = (np.float64(x0) + off * ux).astype(f32)
        y_int = (np.float64(y0) + off * uy).astype(f32)
        if slope == 2:
            return (x_int + (y_int * gradient).astype(f32)).astype(f32), (y_int + (x_int / gradient).astype(f32)).astype(f32)
    if slope == 0:
        return x_int, np.zeros_like(y_int)
    return np.zeros_like(x_int), y_int


LINES = [(0.0, 0.0, 0.02, 0.3), (0.004, 0.11, 0.0123, 0.0371), (0.25, 0.5, 1.0 / 3.0, 0.7)]


@pytest.mark.parametrize("n_off", [1, 40, 1023])
@pytest.mark.parametrize("slope", [0, 1, 2])
def test_boundaries_equal_the_restatement(slope, n_off):
    rng = np.random.default_rng(100 * slope + n_off)
    for x0, y0, x1, y1 in LINES:
        length = float(np.hypot(x1 - x0, y1 - y0))
        for offsets in (np.linspace(-0.3 * length, 1.2 * length, n_off), np.sort(rng.uniform(-length, 2 * length, n_off))):
            got_x, got_y = engine.sweep_boundaries_1d(offsets, slope, x0, y0, x1, y1)
            want_x, want_y = _restated(offsets, slope, x0, y0, x1, y1)
            assert got_x.dtype == f32 and got_y.dtype == f32 and got_x.shape == (n_off,)
            assert got_x.tobytes() == want_x.astype(f32).tobytes()
            assert got_y.tobytes() == want_y.astype(f32).tobytes()
            if slope == 0:
                assert not got_y.any()
            if slope == 1:
                assert not got_x.any()


def test_repeated_offsets_and_none():
    x, y = engine.sweep_boundaries_1d([0.1, 0.1, 0.2], 2, 0.0, 0.0, 0.02, 0.3)
    assert x[0] == x[1] and y[0] == y[1] and x[2] > x[1]
    x, y = engine.sweep_boundaries_1d([], 2, 0.0, 0.0, 0.02, 0.3)
    assert x.shape == (0,) and y.shape == (0,)


def test_argument_errors():
    fn = _lib.lib().ppk_sweep_boundaries_1d
    off = np.asarray([0.0, 0.2, 0.1])
    x = np.zeros(3, dtype=f32)
    y = np.zeros(3, dtype=f32)
    po, px, py = (off.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_float)),
                  y.ctypes.data_as(C.POINTER(C.c_float)))
    assert fn(po, 3, 2, 0.0, 0.0, 0.02, 0.3, px, py) == _lib.ERR_ARG
    assert "sorted" in _lib.last_error()
    with pytest.raises(RuntimeError, match="sorted"):
        engine.sweep_boundaries_1d(off, 2, 0.0, 0.0, 0.02, 0.3)
    off.sort()
    po = off.ctypes.data_as(C.POINTER(C.c_double))
    assert fn(po, 3, 2, 0.0, 0.0, 0.02, 0.3, px, py) == _lib.OK
    assert fn(po, 3, 3, 0.0, 0.0, 0.02, 0.3, px, py) == _lib.ERR_ARG
    assert fn(po, 3, -1, 0.0, 0.0, 0.02, 0.3, px, py) == _lib.ERR_ARG
    assert fn(None, 3, 2, 0.0, 0.0, 0.02, 0.3, px, py) == _lib.ERR_ARG
    assert fn(po, 3, 2, 0.0, 0.0, 0.02, 0.3, None, py) == _lib.ERR_ARG
    assert fn(po, 3, 2, 0.0, 0.0, 0.02, 0.3, px, None) == _lib.ERR_ARG
    many = np.linspace(0.0, 1.0, 1024)
    big = np.zeros(1024, dtype=f32)
    assert fn(many.ctypes.data_as(C.POINTER(C.c_double)), 1024, 2, 0.0, 0.0, 0.02, 0.3,
              big.ctypes.data_as(C.POINTER(C.c_float)), big.ctypes.data_as(C.POINTER(C.c_float))) == _lib.ERR_ARG
