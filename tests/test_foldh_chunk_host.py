"""CPU tests: the 4-plane chunk the holder pair is stored in (tests/foldh_chunk_model.py) -- slot order, plane order,
padding samples zero -- and that it, un-sliced the way engine.SketchDB.foldh_codes un-slices the device copy, is the
model's codes (tests/foldh_model.py) for the planted populations of tests/test_gpu_rank_foldh.py; the 8-plane chunk the
pair used to be stored in un-slices to the same array, its planes 4 .. 7 being zero."""
import types

import numpy as np
import pytest

from foldh_chunk_model import CHUNK_PLANES, chunk_of, codes_of
from foldh_model import foldh_codes_of
from poppunk_amd import engine
from rank_sort_model import order_of
from test_gpu_rank_foldh import CASES, planted


def test_slot_order_plane_order_and_padding():
    n, nk, nbins = 3, 2, 128
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 16, size=(n, nk, nbins)).astype(np.uint16)
    order = np.stack([rng.permutation(nbins) for _ in range(nk)]).astype(np.uint32)
    chunk = chunk_of(codes, order)
    assert chunk.shape == (nk, 2, CHUNK_PLANES, 256) and chunk.dtype == np.uint64
    assert not chunk[..., n:].any()
    for k in range(nk):
        for blk in range(2):
            for plane in range(CHUNK_PLANES):
                for smp in range(n):
                    word = int(chunk[k, blk, plane, smp])
                    for j in range(64):
                        assert (word >> j) & 1 == (int(codes[smp, k, order[k, 64 * blk + j]]) >> plane) & 1
    # the flat layout a launch walks: row (k * s64 + blk) * 4 + plane of [rows][npad]
    flat = chunk.reshape(-1, 256)
    assert np.array_equal(flat[(1 * 2 + 1) * CHUNK_PLANES + 2], chunk[1, 1, 2])
    assert np.array_equal(codes_of(chunk, order, n), codes)


@pytest.mark.parametrize("n,s64,h", CASES)
def test_the_chunk_unsliced_is_the_models_codes(n, s64, h):
    _, bins, eh = planted(n, s64, h)
    order = order_of(eh)
    db = types.SimpleNamespace(n=n, nk=bins.shape[1], sketchsize64=s64)
    for want in foldh_codes_of(bins, h):
        assert want.max() < (1 << CHUNK_PLANES)
        chunk = chunk_of(want, order)
        assert chunk.shape == (bins.shape[1], s64, CHUNK_PLANES, (n + 255) // 256 * 256) and not chunk[..., n:].any()
        eight = chunk_of(want, order, planes=8)
        assert np.array_equal(eight[:, :, :CHUNK_PLANES], chunk) and not eight[:, :, CHUNK_PLANES:].any()
        # engine.SketchDB._codes: un-slice, then undo the sort of the slots
        for raw, planes in ((chunk, CHUNK_PLANES), (eight, 8)):
            slots = engine.SketchDB._unslice_codes(db, raw, planes)
            codes = np.empty_like(slots)
            for k in range(db.nk):
                codes[:, k, order[k]] = slots[:, k]
            assert np.array_equal(codes, want)
        assert np.array_equal(codes_of(chunk, order, n), want)
