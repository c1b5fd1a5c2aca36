"""Numpy statement of the holder pair's stored layout (PPK_CODING_FOLDH, ppk_db_foldh_read), for
tests/test_foldh_chunk_host.py and tests/test_gpu_foldh_chunk.py: a copy is uint64 [nk, sketchsize64, CHUNK_PLANES,
npad] -- word [(k * sketchsize64 + blk) * CHUNK_PLANES + plane][sample] -- whose bit j is bit `plane` of the code in slot
64 * blk + j of k, slot i of k holding stored position order[k, i]; the samples from n up to npad (the next multiple of
256) are zero in every word.  No code of the pair reaches 2^CHUNK_PLANES, so planes 4 .. 7 of the 8-plane coding are
zero and are not stored."""
import numpy as np

CHUNK_PLANES = 4       # PPK_FOLDH_CHUNK_PLANES


def chunk_of(codes, order, planes=CHUNK_PLANES):
    """codes uint16 [n, nk, nbins] by stored position, order [nk, nbins] -> uint64 [nk, nbins / 64, planes, npad]"""
    n, nk, nbins = codes.shape
    npad = (n + 255) // 256 * 256
    out = np.zeros((nk, nbins // 64, planes, npad), dtype=np.uint64)
    weight = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for k in range(nk):
        slots = codes[:, k, order[k].astype(np.int64)].reshape(n, nbins // 64, 64)
        for b in range(planes):
            bits = ((slots >> b) & 1).astype(np.uint64)
            out[k, :, b, :n] = np.bitwise_or.reduce(bits * weight, axis=2).T
    return out


def codes_of(chunk, order, n):
    """the inverse: uint16 [n, nk, nbins] codes by stored position"""
    nk, s64, planes, _ = chunk.shape
    slots = np.zeros((n, nk, s64, 64), dtype=np.uint16)
    for b in range(planes):
        for j in range(64):
            slots[..., j] |= (((chunk[:, :, b, :n] >> np.uint64(j)) & np.uint64(1)).astype(np.uint16) << b).transpose(2, 0, 1)
    slots = slots.reshape(n, nk, 64 * s64)
    codes = np.empty_like(slots)
    for k in range(nk):
        codes[:, k, order[k].astype(np.int64)] = slots[:, k]
    return codes

