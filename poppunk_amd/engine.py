"""Device-level engine: resident sketch databases, kernel launches on torch
tensors/streams, and the band-sharded multi-GPU path.

PyTorch is plumbing here (device memory, streams, torch.distributed over
RCCL); all arithmetic happens in libppk_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib

FLAG_RANDOM_CORRECT = _lib.FLAG_RANDOM_CORRECT
FLAG_JACCARD = _lib.FLAG_JACCARD
FLAG_COUNTS = _lib.FLAG_COUNTS


def _torch():
    import torch
    return torch


def _stream_ptr(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the frame every device call below goes through ------------------------------------------------
def _dev_call(name, dev, *args, then=(), arg_error=None, accept=()):
    """`name(*args, stream, *then)` on device `dev`: inside torch.cuda.device(dev), with every tensor (anything that
    has a data_ptr) as its address and the device's current stream -- read now, never kept: callers switch streams --
    after the arguments (`then`: what the two create calls declare behind the stream).  Host arrays, scalars, None
    and the status (`arg_error`, `accept`) are `_lib.call`'s.  Addresses go in as plain integers, which ctypes turns
    into the `void *` SIGNATURES declares exactly as it does a c_void_p, without an object per argument and call."""
    cuda = _torch().cuda
    scope = cuda.device(dev)        # (resolves `dev` -- an index, a torch.device, "cuda:0" -- once: .idx)
    with scope:
        return _lib.call(name, *[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args],
                         cuda.current_stream(scope.idx).cuda_stream, *then, arg_error=arg_error, accept=accept)


def _check_tensor(t, message, dtype, shape=None, dim=None, numel=None, like=None, contiguous=True):
    """TypeError(message) unless t is a CUDA tensor of `dtype` (one, or a tuple to choose from), contiguous, with
    `dim` dimensions (one, or a tuple), the sizes of `shape` (None: any size) or `numel` elements, on the device of
    `like`."""
    ok = (t.is_cuda and (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype))
          and (not contiguous or t.is_contiguous())
          and (dim is None or (t.dim() in dim if type(dim) is tuple else t.dim() == dim))
          and (numel is None or int(t.numel()) == numel)
          and (like is None or t.device == like.device))
    if ok and shape is not None:
        have = t.shape
        ok = len(have) == len(shape)
        for want, size in zip(shape, have):
            ok = ok and (want is None or want == size)
    if not ok:
        raise TypeError(message)


def _cap_guess(n):
    """The first capacity of a data-dependent list out of n rows (a short guess costs one exact re-run)."""
    return min(n, max(1 << 20, n // 8))


def _neighbour_outputs(n, dev):
    """(i int64, j int64, dist float32) of n entries each: the neighbour lists as get_kNN_distances returns them."""
    torch = _torch()
    return (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev))


def rows_in_band(n_ref, n_qry, q_begin, q_end):
    return int(_lib.lib().ppk_rows_in_band(n_ref, n_qry, q_begin, q_end))


def band_split(n_ref, n_qry, n_parts):
    """Query-axis band edges giving n_parts (nearly) equal pair counts (multiples of 64)."""
    bounds = (C.c_size_t * (n_parts + 1))()
    _lib.call("ppk_band_split", n_ref, n_qry, n_parts, bounds)
    return [int(b) for b in bounds]


def band_split_weighted(n_ref, n_qry, weights):
    """Query-axis band edges giving band i the share weights[i] / sum(weights) of the pair space
    (edges on multiples of 64 queries, like ppk_band_split; equal weights reproduce it).  Self:
    the rows before query q number q*n - q(q+1)/2, inverted in closed form."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or len(w) < 1 or not np.all(np.isfinite(w)) or np.any(w < 0) or w.sum() <= 0:
        raise ValueError("weights must be non-negative, finite and not all zero")
    nq = n_qry if n_qry else n_ref
    total = float(rows_in_band(n_ref, n_qry, 0, nq))
    cum = np.cumsum(w) / w.sum()
    bounds = [0]
    for p in range(len(w) - 1):
        target = total * float(cum[p])
        if n_qry == 0:
            b = 2.0 * n_ref - 1.0
            disc = max(b * b - 8.0 * target, 0.0)
            q = int((b - disc ** 0.5) / 2.0)
        else:
            q = int(target / float(n_ref))
        q = (q + 32) // 64 * 64
        bounds.append(max(min(q, nq), bounds[-1]))
    bounds.append(nq)
    return bounds


class SketchDB:
    """One sample list's bin-sketches resident in HBM on one GPU (ppk_db).

    sketches: numpy uint64 [n, nk, sketchsize64*bbits] (host) or a torch int64 CUDA
    tensor of the same shape already on `device`.
    clusters: optional uint16 [n] random-match cluster ids.
    """

    def __init__(self, sketches, sketchsize64, bbits, clusters=None, device=0):
        torch = _torch()
        self.device = int(device)
        self.sketchsize64 = int(sketchsize64)
        self.bbits = int(bbits)
        self._h = C.c_void_p()
        on_dev = hasattr(sketches, "is_cuda")
        if on_dev:
            if not sketches.is_cuda or sketches.dtype != torch.int64 or not sketches.is_contiguous():
                raise ValueError("device sketches must be a contiguous int64 CUDA tensor")
            if sketches.device.index != self.device:
                raise ValueError("sketch tensor is on a different device")
            n, nk, words = sketches.shape
        else:
            sketches = np.ascontiguousarray(sketches, dtype=np.uint64)
            if sketches.ndim != 3:
                raise ValueError("sketches must be [n, nk, sketchsize64*bbits]")
            n, nk, words = sketches.shape
        if words != self.sketchsize64 * self.bbits:
            raise ValueError("sketch word count %d != sketchsize64*bbits = %d"
                             % (words, self.sketchsize64 * self.bbits))
        self.n, self.nk = int(n), int(nk)
        self._clu_keep = None
        if clusters is not None:
            if on_dev:
                c = clusters.to(device="cuda:%d" % self.device, dtype=torch.int16).contiguous()
            else:
                c = np.ascontiguousarray(clusters, dtype=np.uint16)
                if c.shape != (n,):
                    raise ValueError("clusters must be [n]")
            self._clu_keep = c
        _dev_call("ppk_db_create", self.device, self.device, sketches, n, nk, self.sketchsize64, self.bbits,
                  self._clu_keep, 1 if on_dev else 0, then=(C.byref(self._h),))
        if on_dev:
            torch.cuda.current_stream(self.device).synchronize()   # source tensor may be freed

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().ppk_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n

    @property
    def rank_planes(self):
        """Bit-planes of the database's rank-coded copy (8, 10 or 12), 0 without one (ppk_db_rank_planes)."""
        return int(_lib.lib().ppk_db_rank_planes(self._h))

    def rank_block_planes(self):
        """Planes a self job compares per 64-bin block of the rank-coded copy (ppk_db_rank_block_planes): uint8
        [nk, sketchsize64], rank_planes or -- where no position of the block holds more than 2^(rank_planes - 1)
        distinct values -- rank_planes - 1.  The database's own flags: option "rank_short" 0 does not change them."""
        return self._per_block("ppk_db_rank_block_planes")

    def _per_block(self, fn, per_block=1, dtype=np.uint8):
        """[nk, per_block * sketchsize64] from one of the ppk_db_*_block_planes / _stream_planes / _position_order
        accessors"""
        out = np.empty((self.nk, per_block * self.sketchsize64), dtype=dtype)
        _lib.call(fn, self._h, out, out.size)
        return out

    def _codes(self, fn, planes, which=None, order=None):
        """One coded copy (ppk_db_*_read) un-bitsliced; with `order`, the sort of its slots undone."""
        npad = (self.n + 255) // 256 * 256
        raw = np.empty((self.nk, self.sketchsize64, max(planes, 1), npad), dtype=np.uint64)
        _lib.call(fn, self._h, *(() if which is None else (int(which),)), raw,
                  self.nk * self.sketchsize64 * planes * npad)
        slots = self._unslice_codes(raw, planes)
        if order is None:
            return slots
        codes = np.empty_like(slots)
        for k in range(self.nk):
            codes[:, k, order[k]] = slots[:, k]
        return codes

    def _bucketed(self, size_fn, read_fn, dtype):
        """(offsets uint32, list) of a coding's bucketed corrections (ppk_db_*_events / _entries and their _read)"""
        nb = C.c_size_t(0)
        count = int(getattr(_lib.lib(), size_fn)(self._h, C.byref(nb)))
        off = np.zeros(nb.value + 1, dtype=np.uint32)
        items = np.zeros(count, dtype=dtype)
        _lib.call(read_fn, self._h, off, off.size, items if count else None, count)
        return off, items

    def _unslice_codes(self, raw, planes):
        """coded planes [nk, sketchsize64, planes, npad] uint64 -> uint16 [n, nk, 64 * sketchsize64] codes"""
        bits = np.unpackbits(raw[..., :self.n].view(np.uint8).reshape(self.nk, self.sketchsize64, planes, self.n, 8),
                             axis=-1, bitorder="little")      # [k, blk, plane, sample, 64 bins]
        codes = np.zeros((self.nk, self.sketchsize64, self.n, 64), dtype=np.uint16)
        for b in range(planes):
            codes |= bits[:, :, b].astype(np.uint16) << b
        return np.ascontiguousarray(codes.transpose(2, 0, 1, 3)).reshape(self.n, self.nk, 64 * self.sketchsize64)

    def rank_codes(self):
        """The rank-coded copy un-bitsliced (tests): uint16 [n, nk, 64 * sketchsize64] codes."""
        return self._codes("ppk_db_rank_read", self.rank_planes)

    @property
    def fold_planes(self):
        """Bit-planes of the database's folded pair of coded copies (8, 10 or 12), 0 without one (ppk_db_fold_planes)."""
        return int(_lib.lib().ppk_db_fold_planes(self._h))

    def fold_block_planes(self):
        """Planes a self job compares per 64-bin block of the folded pair (ppk_db_fold_block_planes): uint8
        [nk, sketchsize64], fold_planes or -- where no position of the block spans more than 2^(fold_planes - 1)
        codes -- fold_planes - 1."""
        return self._per_block("ppk_db_fold_block_planes")

    def fold_codes(self, which):
        """One copy of the folded pair un-bitsliced (tests), 0 the ref side, 1 the query side: uint16
        [n, nk, 64 * sketchsize64] codes."""
        return self._codes("ppk_db_fold_read", self.fold_planes, which)

    @property
    def fold2_planes(self):
        """Bit-planes of the database's two-holder pair of coded copies (8), 0 without one (ppk_db_fold2_planes)."""
        return int(_lib.lib().ppk_db_fold2_planes(self._h))

    def fold2_block_planes(self):
        """The 8 / 7 plane rule on the 64-bin blocks of the two-holder pair as the sketches store them
        (ppk_db_fold2_block_planes): uint8 [nk, sketchsize64].  What a self job compares: fold2_stream_planes()."""
        return self._per_block("ppk_db_fold2_block_planes")

    def fold2_stream_planes(self):
        """Planes a self job compares per block of the two-holder pair's sorted positions, under the options in force
        (ppk_db_fold2_stream_planes): uint8 [nk, sketchsize64] of 8, 7 or 6."""
        return self._per_block("ppk_db_fold2_stream_planes")

    def fold2_position_order(self):
        """The stored position each slot of the two-holder pair holds (ppk_db_fold2_position_order): uint32
        [nk, 64 * sketchsize64], per k a permutation (the identity under option "fold2_sort" 0)."""
        return self._per_block("ppk_db_fold2_position_order", 64, np.uint32)

    def fold2_codes(self, which):
        """One copy of the two-holder pair un-bitsliced (tests), 0 the ref side, 1 the query side: uint16
        [n, nk, 64 * sketchsize64] codes, in stored position order (the sort of fold2_position_order() undone)."""
        return self._codes("ppk_db_fold2_read", self.fold2_planes, which, self.fold2_position_order())

    def fold2_events(self):
        """The event list of the two-holder pair (ppk_db_fold2_events_read): (offsets uint32 [npad / 32, npad / 256]
        flattened + 1, events uint16).  Bucket (lo // 32) * (npad // 256) + hi // 256 holds
        events[offsets[b]:offsets[b + 1]], each hi % 256 | (lo % 32) << 8 | k << 13, in no order within a bucket."""
        return self._bucketed("ppk_db_fold2_events", "ppk_db_fold2_events_read", np.uint16)

    def foldh_holders(self):
        """The holder bound H of the database's holder pair, 0 without one (ppk_db_foldh_holders): every bin value
        with at most H holders is coded 0 / 1 there and what its pairs are owed is kept in foldh_entries()."""
        return int(_lib.lib().ppk_db_foldh_holders(self._h))

    def foldh_stream_planes(self):
        """Planes a self job compares per block of the holder pair's sorted positions, under the options in force
        (ppk_db_foldh_stream_planes): uint8 [nk, sketchsize64] of 4, 3 or 2."""
        return self._per_block("ppk_db_foldh_stream_planes")

    def foldh_position_order(self):
        """The stored position each slot of the holder pair holds (ppk_db_foldh_position_order): uint32
        [nk, 64 * sketchsize64], per k a permutation."""
        return self._per_block("ppk_db_foldh_position_order", 64, np.uint32)

    def foldh_codes(self, which):
        """One copy of the holder pair un-bitsliced (tests), 0 the ref side, 1 the query side: uint16
        [n, nk, 64 * sketchsize64] codes, in stored position order (the sort of foldh_position_order() undone)."""
        planes = int(_lib.lib().ppk_db_foldh_chunk_planes(self._h))      # (the planes a block stores: 4)
        return self._codes("ppk_db_foldh_read", planes, which, self.foldh_position_order())

    def foldh_entries(self):
        """What the holder pair's compare owes (ppk_db_foldh_entries_read): (offsets uint32 [npad / 32, npad / 256]
        flattened + 1, entries uint32).  Bucket (lo // 32) * (npad // 256) + hi // 256 holds
        entries[offsets[b]:offsets[b + 1]], each hi % 256 | (lo % 32) << 8 | k << 13 | count << 16, one per (pair, k)
        with a non-zero count, in no order within a bucket."""
        return self._bucketed("ppk_db_foldh_entries", "ppk_db_foldh_entries_read", np.uint32)

    def rank_counts(self):
        """What the count pass of the coded copies found (ppk_db_rank_counts), None where none ran: a dict of the
        maxima over all positions "D", "E", "E2", per (k, block) "block_D", "block_E", "block_E2" [nk, sketchsize64],
        "two_max" (most two-holder values of a position), "two_total" and "pair_cap_hit"."""
        words = int(_lib.lib().ppk_db_rank_counts(self._h, None, 0))
        if not words:
            return None
        raw = np.zeros(words, dtype=np.uint32)
        _lib.lib().ppk_db_rank_counts(self._h, raw.ctypes.data, raw.size)      # (returns the word count, no status)
        seg = 1 + self.nk * self.sketchsize64
        out = {}
        for i, name in enumerate(("D", "E", "E2")):
            out[name] = int(raw[i * seg])
            out["block_" + name] = raw[i * seg + 1:(i + 1) * seg].reshape(self.nk, self.sketchsize64).copy()
        out["two_max"], out["two_total"], out["pair_cap_hit"] = (int(x) for x in raw[3 * seg:3 * seg + 3])
        return out


def _prep_tables(kmers, random_tbl, nk):
    """(kmers int32 [nk], random table float32 [nk, n_clu, n_clu] or None, n_clu) as the kernel-1 calls take them."""
    kmers = np.ascontiguousarray(kmers, dtype=np.int32)
    if kmers.shape != (nk,):
        raise ValueError("klist length %d does not match the sketches' %d k-mer lengths"
                         % (kmers.size, nk))
    n_clu = 0
    if random_tbl is not None:
        random_tbl = np.ascontiguousarray(random_tbl, dtype=np.float32)
        if random_tbl.ndim != 3 or random_tbl.shape[0] != nk or random_tbl.shape[1] != random_tbl.shape[2]:
            raise ValueError("random table must be [nk, n_clu, n_clu]")
        n_clu = random_tbl.shape[1]
    return kmers, random_tbl, n_clu


def _check_pair(ref, qry):
    if qry is not None and (qry.nk != ref.nk or qry.sketchsize64 != ref.sketchsize64
                            or qry.bbits != ref.bbits or qry.device != ref.device):
        raise ValueError("ref and query databases are incompatible")


def dist(ref, qry=None, kmers=None, random_tbl=None, random_correct=True, jaccard=False,
         counts=False, q_begin=0, q_end=None, out=None, n_failed=None):
    """Enqueue kernel 1 for query rows [q_begin, q_end) on the current stream.

    Returns (out, n_failed): out is a CUDA tensor float32 [rows,2] (core, accessory),
    float32 [rows,nk] (jaccard) or int32 [rows,nk] (counts); n_failed a 1-element
    int64 CUDA tensor (pairs with < 2 usable k-mer lengths).  A caller-provided `n_failed`
    is ADDED to (a job that launches band after band keeps one counter instead of paying a
    fill kernel per launch).
    """
    torch = _torch()
    _check_pair(ref, qry)
    nq = qry.n if qry is not None else ref.n
    q_end = nq if q_end is None else int(q_end)
    kmers, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    rows = rows_in_band(ref.n, qry.n if qry is not None else 0, q_begin, q_end)
    flags = (FLAG_RANDOM_CORRECT if random_correct else 0) | (FLAG_JACCARD if jaccard else 0) \
        | (FLAG_COUNTS if counts else 0)
    cols = ref.nk if (jaccard or counts) else 2
    dev = "cuda:%d" % ref.device
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.int32 if counts else torch.float32, device=dev)
    elif out.numel() != rows * cols or not out.is_contiguous() or out.element_size() != 4:
        raise ValueError("out has the wrong size")
    if n_failed is None:
        n_failed = torch.zeros(1, dtype=torch.int64, device=dev)
    _dev_call("ppk_dist_dev", ref.device, ref._h, qry._h if qry is not None else None, kmers, random_tbl, n_clu,
              flags, q_begin, q_end, out, n_failed)
    return out, n_failed


def _fused_edges(name, ref, qry, kmers, random_tbl, random_correct, q_begin, q_end, cap, *test):
    """The fused kernel-1 edge calls (line boundary / BGMM): capacity guess, exact re-run when it was short.
    `name(ref_h, qry_h, kmers, tbl, n_clu, flags, q_begin, q_end, *test, d_edges, cap, d_n_edges, d_n_failed, stream)`."""
    torch = _torch()
    _check_pair(ref, qry)
    nq = qry.n if qry is not None else ref.n
    q_end = nq if q_end is None else int(q_end)
    kmers, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    rows = rows_in_band(ref.n, qry.n if qry is not None else 0, q_begin, q_end)
    flags = FLAG_RANDOM_CORRECT if random_correct else 0
    dev = torch.device("cuda:%d" % ref.device)
    if cap is None:
        cap = _cap_guess(rows)
    n_failed = torch.zeros(1, dtype=torch.int64, device=dev)

    def launch(edges, c, n_edges):
        n_failed.zero_()
        _dev_call(name, dev, ref._h, qry._h if qry is not None else None, kmers, random_tbl, n_clu, flags, q_begin,
                  q_end, *test, edges, c, n_edges, n_failed)
    return _edges_dev(launch, dev, cap), n_failed


def dist_edges(ref, qry=None, kmers=None, random_tbl=None, random_correct=True, slope=2,
               x_max=0.0, y_max=0.0, scale=(1.0, 1.0), inclusive=True, q_begin=0, q_end=None,
               cap=None):
    """Fused kernel 1 + boundary + compaction.  Returns (edges int64 [n_edges,2] CUDA, n_failed).

    The edge count is data dependent: the call runs with a capacity guess and is
    re-run with the exact size only if the guess was too small."""
    return _fused_edges("ppk_dist_edges_dev", ref, qry, kmers, random_tbl, random_correct, q_begin, q_end, cap,
                        int(slope), float(x_max), float(y_max), float(scale[0]), float(scale[1]),
                        1 if inclusive else 0)


def _fused_edges_rows(name, ref, qry, kmers, random_tbl, random_correct, q_begin, q_end, cap, *test):
    """The fused edge calls that also return every edge's unscaled (core, accessory) row: _fused_edges with a float32
    [cap, 2] buffer next to the edges; the exact re-run refills both (a short run leaves the rows unspecified).
    Returns (edges, rows, n_failed)."""
    torch = _torch()
    rows_of = {}

    def with_rows(call, edges, c, n_edges, n_failed):
        rows = torch.empty((max(c, 1), 2), dtype=torch.float32, device=edges.device)
        rows_of["rows"] = rows
        call(edges, rows, c, n_edges, n_failed)

    _check_pair(ref, qry)
    nq = qry.n if qry is not None else ref.n
    q_end = nq if q_end is None else int(q_end)
    kmers, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    n_rows = rows_in_band(ref.n, qry.n if qry is not None else 0, q_begin, q_end)
    flags = FLAG_RANDOM_CORRECT if random_correct else 0
    dev = torch.device("cuda:%d" % ref.device)
    if cap is None:
        cap = _cap_guess(n_rows)
    n_failed = torch.zeros(1, dtype=torch.int64, device=dev)

    def launch(edges, c, n_edges):
        n_failed.zero_()
        with_rows(lambda e, r, cc, ne, nf: _dev_call(name, dev, ref._h, qry._h if qry is not None else None, kmers,
                                                     random_tbl, n_clu, flags, q_begin, q_end, *test, e, r, cc, ne, nf),
                  edges, c, n_edges, n_failed)
    edges = _edges_dev(launch, dev, cap)
    return edges, rows_of["rows"][:edges.shape[0]], n_failed


def dist_edges_rows(ref, qry=None, kmers=None, random_tbl=None, random_correct=True, slope=2,
                    x_max=0.0, y_max=0.0, scale=(1.0, 1.0), inclusive=True, q_begin=0, q_end=None,
                    cap=None):
    """dist_edges, and with every edge its distances (ppk_dist_edges_rows_dev).  Returns (edges int64
    [n_edges, 2], rows float32 [n_edges, 2], n_failed): rows[e] is the UNSCALED (core, accessory) of edge e, bit for bit
    the row `dist` writes for that pair; `scale` only enters the boundary test."""
    return _fused_edges_rows("ppk_dist_edges_rows_dev", ref, qry, kmers, random_tbl, random_correct, q_begin, q_end,
                             cap, int(slope), float(x_max), float(y_max), float(scale[0]), float(scale[1]),
                             1 if inclusive else 0)


def _host_edges(name, refs, qrys, kmers, random_tbl, random_correct, cap, *test):
    """The multi-device host edge calls (line boundary / BGMM): one SketchDB per device (or a single one), a host int64
    [m, 2] array, the parked list fetched when `cap` was too small.
    `name(refs_h, qrys_h, n_dev, kmers, tbl, n_clu, flags, *test, out, cap, byref(n_edges), byref(n_failed))`."""
    refs = [refs] if isinstance(refs, SketchDB) else list(refs)
    if qrys is not None:
        qrys = [qrys] if isinstance(qrys, SketchDB) else list(qrys)
        if len(qrys) != len(refs):
            raise ValueError("one query database per reference database")
        for r, q in zip(refs, qrys):
            _check_pair(r, q)
    ref = refs[0]
    kmers, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    n_qry = qrys[0].n if qrys is not None else 0
    rows = rows_in_band(ref.n, n_qry, 0, n_qry if qrys is not None else ref.n)
    if cap is None:
        cap = _cap_guess(rows)
    rh = (C.c_void_p * len(refs))(*[r._h.value for r in refs])
    qh = (C.c_void_p * len(refs))(*[q._h.value for q in qrys]) if qrys is not None else None
    out = np.empty((max(int(cap), 1), 2), dtype=np.int64)
    n_edges = C.c_size_t(0)
    n_failed = C.c_ulonglong(0)
    rc = _lib.call(name, rh, qh, len(refs), kmers, random_tbl, n_clu, FLAG_RANDOM_CORRECT if random_correct else 0,
                   *test, out, int(cap), C.byref(n_edges), C.byref(n_failed), accept=(_lib.ERR_CAPACITY,))
    if rc == _lib.ERR_CAPACITY:
        out = np.empty((n_edges.value, 2), dtype=np.int64)
        _lib.call("ppk_parked_fetch", out, None, None, n_edges.value, None, what=name)
    return out[:n_edges.value], int(n_failed.value)


def edges_host(refs, qrys=None, kmers=None, random_tbl=None, random_correct=True, slope=2, x_max=0.0,
               y_max=0.0, scale=(1.0, 1.0), inclusive=True, cap=None):
    """ppk_query_edges_dbs: the edge list of the whole matrix as a host int64 [m, 2] array, computed by
    every device that holds a copy of the database (`refs` / `qrys`: one SketchDB per device, or a single
    SketchDB), each on its band of rows, one worker thread per device inside the library.
    Returns (edges, n_failed)."""
    return _host_edges("ppk_query_edges_dbs", refs, qrys, kmers, random_tbl, random_correct, cap, int(slope),
                       float(x_max), float(y_max), float(scale[0]), float(scale[1]), 1 if inclusive else 0)


def _check_dist_tensor(dist_t):
    _check_tensor(dist_t, "distMat must be a C-contiguous float32 [n,2] CUDA tensor", _torch().float32, (None, 2))


def bgmm_assign_dev(dist_t, model, labels=True, values=False):
    """BGMMFit.assign on a resident float32 [n,2] CUDA tensor with a prepared model (`_lib.Bgmm`).
    Returns (labels int32 [n] or None, responsibilities float32 [n, K] or None)."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    if not (labels or values):
        raise ValueError("ask for labels, responsibilities or both")
    n = dist_t.shape[0]
    lab = torch.empty(n, dtype=torch.int32, device=dist_t.device) if labels else None
    resp = torch.empty((n, model.K), dtype=torch.float32, device=dist_t.device) if values else None
    _dev_call("ppk_bgmm_assign_dev", dist_t.device, dist_t, n, C.byref(model), lab, resp)
    return lab, resp


def _edges_dev(launch, device, cap):
    """Run an edge-list call, `launch(edges, cap, n_edges)`, with a capacity guess, once more with the exact size if
    the guess was short."""
    torch = _torch()
    while True:
        edges = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=device)
        n_edges = torch.zeros(1, dtype=torch.int64, device=device)
        launch(edges, cap, n_edges)
        m = int(n_edges.item())
        if m <= cap:
            return edges[:m]
        cap = m


def _row_edges_dev(name, dist_t, cap, *test):
    """The edge list of the rows of a resident [n, 2] matrix that pass a test:
    `name(dist, n, *test, d_edges, cap, d_n_edges, stream)` through _edges_dev."""
    _check_dist_tensor(dist_t)
    n = dist_t.shape[0]
    return _edges_dev(lambda e, c, ne: _dev_call(name, dist_t.device, dist_t, n, *test, e, c, ne), dist_t.device,
                      _cap_guess(n) if cap is None else cap)


def bgmm_edges_dev(dist_t, model, n_ref=0, int_offset=0, cap=None):
    """Rows labelled model.within_label -> int64 [m,2] edges in generateTuples order (n_ref 0: self)."""
    return _row_edges_dev("ppk_bgmm_edges_dev", dist_t, cap, int(n_ref), C.byref(model), int(int_offset))


# ---- BGMM fit (include/ppk.h "BGMM fit") --------------------------------------------------------
def bgmm_fit_params(K, **overrides):
    """`_lib.BgmmFitParams` with fit2dMultiGaussian's values (PopPUNK/bgmm.py:38-43); keyword arguments replace
    fields (`mean_prior` a pair).  ValueError for values outside their ranges (K outside [1, 16], ...)."""
    p = _lib.BgmmFitParams()
    _lib.call("ppk_bgmm_fit_params_default", int(K), C.byref(p), arg_error=ValueError)
    for k, v in overrides.items():
        if k == "mean_prior":
            p.mean_prior[0], p.mean_prior[1] = float(v[0]), float(v[1])
        elif k in ("max_iter", "n_init"):
            setattr(p, k, int(v))
        elif k in ("weight_concentration_prior", "mean_precision_prior", "degrees_of_freedom_prior", "reg_covar", "tol"):
            setattr(p, k, float(v))
        else:
            raise TypeError("unknown BGMM fit parameter %r" % k)
    return p


def _fit_scale(scale):
    """(the two float32 scales, a pointer to them): the array goes to the frame, the pointer to raw library calls
    (tests make some)."""
    s = np.ascontiguousarray(np.asarray(scale, dtype=np.float32).reshape(2))
    return s, s.ctypes.data_as(C.POINTER(C.c_float))


def _check_index_tensor(index_t, dist_t):
    """The length of the optional list of training rows (0 without one), after checking it."""
    if index_t is None:
        return 0
    _check_tensor(index_t, "index must be a contiguous int64 [m] CUDA tensor on the matrix's device", _torch().int64,
                  dim=1, like=dist_t)
    return index_t.shape[0]


def bgmm_stats_dev(dist_t, state, scale, index_t=None):
    """One E-step + statistics pass (ppk_bgmm_stats_dev) from a `_lib.BgmmState`: float64 CUDA [K, 7], per component
    S r, S r dx, S r dy, S r dx dx, S r dx dy, S r dy dy, S r log r about the state's means."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    ni = _check_index_tensor(index_t, dist_t)
    out = torch.empty((state.K, _lib.BGMM_FIT_STATS), dtype=torch.float64, device=dist_t.device)
    _dev_call("ppk_bgmm_stats_dev", dist_t.device, dist_t, dist_t.shape[0], index_t, ni, _fit_scale(scale)[0],
              C.byref(state), out, arg_error=ValueError)
    return out


def bgmm_kmeans_dev(dist_t, centres, scale, labels_t, index_t=None):
    """One pass of the own initialisation (ppk_bgmm_kmeans_dev): `labels_t` (int32 CUDA, one per training row) is
    rewritten with the nearest of `centres` [K, 2]; returns (sums float64 CUDA [K, 7] about the centres, number of
    labels that changed as an int32 CUDA tensor [1])."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    ni = _check_index_tensor(index_t, dist_t)
    n = ni if index_t is not None else dist_t.shape[0]
    _check_tensor(labels_t, "labels must be a contiguous int32 CUDA tensor with one entry per training row",
                  torch.int32, (n,))
    c = np.ascontiguousarray(centres, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError("centres must be [K, 2]")
    out = torch.empty((c.shape[0], _lib.BGMM_FIT_STATS), dtype=torch.float64, device=dist_t.device)
    changed = torch.zeros(1, dtype=torch.int32, device=dist_t.device)
    _dev_call("ppk_bgmm_kmeans_dev", dist_t.device, dist_t, dist_t.shape[0], index_t, ni, _fit_scale(scale)[0],
              c.shape[0], c, labels_t, out, changed, arg_error=ValueError)
    return out, changed


def _fit_centres(init_centres, params):
    if init_centres is None:
        return None
    c = np.ascontiguousarray(init_centres, dtype=np.float64)
    if c.shape != (params.n_init, params.K, 2):
        raise ValueError("init_centres must be [n_init, K, 2]")
    return c


def bgmm_fit_dev(dist_t, scale, params, index_t=None, init_labels_t=None, init_centres=None):
    """The fit on a resident float32 [n, 2] CUDA matrix (ppk_bgmm_fit_dev): every row, or the rows `index_t` names.
    Exactly one of `init_labels_t` (int32 CUDA, one per training row) and `init_centres` ([n_init, K, 2]).  Returns a
    `bgmm.FitResult`; ValueError for what the header lists as PPK_ERR_ARG."""
    from . import bgmm
    torch = _torch()
    _check_dist_tensor(dist_t)
    ni = _check_index_tensor(index_t, dist_t)
    n = ni if index_t is not None else dist_t.shape[0]
    if init_labels_t is not None:
        _check_tensor(init_labels_t, "init_labels must be a contiguous int32 CUDA tensor with one entry per training "
                      "row", torch.int32, (n,))
    c = _fit_centres(init_centres, params)
    res = _lib.BgmmFitResult()
    _dev_call("ppk_bgmm_fit_dev", dist_t.device, dist_t, dist_t.shape[0], index_t, ni, _fit_scale(scale)[0],
              init_labels_t, c, C.byref(params), C.byref(res), arg_error=ValueError)
    return bgmm.FitResult(res)


def bgmm_fit(X, scale, params, index=None, init_labels=None, init_centres=None, device_id=0):
    """The same from host arrays (ppk_bgmm_fit; blocking): X float32 [n, 2], `index` int64 positions or None."""
    from . import bgmm
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] != 2:
        raise ValueError("X must be [n, 2] (core, accessory)")
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64)
    lab = None if init_labels is None else np.ascontiguousarray(init_labels, dtype=np.int32)
    n = X.shape[0] if idx is None else idx.shape[0]
    if lab is not None and lab.shape != (n,):
        raise ValueError("init_labels must have one entry per training row")
    c = _fit_centres(init_centres, params)
    res = _lib.BgmmFitResult()
    _lib.call("ppk_bgmm_fit", X, X.shape[0], idx, 0 if idx is None else idx.shape[0], _fit_scale(scale)[0], lab, c,
              C.byref(params), int(device_id), C.byref(res), arg_error=ValueError)
    return bgmm.FitResult(res)


def generate_tuples_dev(assign_t, within_label, self_comparison=True, num_ref=0, int_offset=0, cap=None):
    """poppunk_refine.generateTuples on a resident int32 [n] CUDA tensor -> int64 [m,2]."""
    _check_tensor(assign_t, "assignments must be a contiguous int32 CUDA tensor", _torch().int32)
    n = assign_t.shape[0]
    return _edges_dev(lambda e, c, ne: _dev_call(
        "ppk_generate_tuples_dev", assign_t.device, assign_t, n, int(within_label), 1 if self_comparison else 0,
        int(num_ref), int(int_offset), e, c, ne), assign_t.device, _cap_guess(n) if cap is None else cap)


def _check_points_tensor(pts_t):
    _check_tensor(pts_t, "points must be a C-contiguous float32 [n,2] CUDA tensor", _torch().float32, (None, 2))


def dbscan_core_dev(pts_t, min_samples):
    """Squared core distances of scaled training points (ppk_dbscan_core_dev): float64 [n], the
    min_samples-th smallest squared distance to another point, bit for bit np.partition's of the float64 row."""
    torch = _torch()
    _check_points_tensor(pts_t)
    n = pts_t.shape[0]
    core2 = torch.empty(n, dtype=torch.float64, device=pts_t.device)
    _dev_call("ppk_dbscan_core_dev", pts_t.device, pts_t, n, int(min_samples), core2, arg_error=ValueError)
    return core2


def dbscan_mst_dev(pts_t, core2_t):
    """The minimum spanning tree of the mutual-reachability graph under the total order (mr2, lo, hi)
    (ppk_dbscan_mst_dev).  Returns (a int32 [n-1], b int32 [n-1], mr2 float64 [n-1]), sorted by that order."""
    torch = _torch()
    _check_points_tensor(pts_t)
    n = pts_t.shape[0]
    _check_tensor(core2_t, "core2 must be a contiguous float64 [n] CUDA tensor", torch.float64, (n,))
    dev = pts_t.device
    a = torch.empty(max(n - 1, 1), dtype=torch.int32, device=dev)
    b = torch.empty(max(n - 1, 1), dtype=torch.int32, device=dev)
    w = torch.empty(max(n - 1, 1), dtype=torch.float64, device=dev)
    _dev_call("ppk_dbscan_mst_dev", dev, pts_t, core2_t, n, a, b, w)
    return a[:n - 1], b[:n - 1], w[:n - 1]


def dbscan_assign_dev(dist_t, handle):
    """DBSCANFit.assign on a resident float32 [n,2] CUDA tensor with a model handle (ppk_dbscan_create): int32 [n]."""
    _check_dist_tensor(dist_t)
    n = dist_t.shape[0]
    lab = _torch().empty(n, dtype=_torch().int32, device=dist_t.device)
    _dev_call("ppk_dbscan_assign_dev", dist_t.device, dist_t, n, handle, lab)
    return lab


def dbscan_edges_dev(dist_t, handle, n_ref=0, int_offset=0, cap=None):
    """Rows assigned the model's within-strain label -> int64 [m,2] edges in generateTuples order (n_ref 0: self)."""
    return _row_edges_dev("ppk_dbscan_edges_dev", dist_t, cap, int(n_ref), handle, int(int_offset))


def dist_bgmm_edges(ref, qry=None, kmers=None, random_tbl=None, model=None, random_correct=True, q_begin=0,
                    q_end=None, cap=None):
    """Fused kernel 1 + BGMM assignment + compaction (ppk_dist_bgmm_edges_dev).  Returns (edges int64 [n_edges,2]
    CUDA, n_failed); capacity guess, exact re-run when it was short (as dist_edges)."""
    if model is None:
        raise ValueError("a prepared BGMM model is needed")
    return _fused_edges("ppk_dist_bgmm_edges_dev", ref, qry, kmers, random_tbl, random_correct, q_begin, q_end, cap,
                        C.byref(model))


def dist_bgmm_edges_rows(ref, qry=None, kmers=None, random_tbl=None, model=None, random_correct=True, q_begin=0,
                         q_end=None, cap=None):
    """dist_bgmm_edges, and with every edge its (core, accessory) row (ppk_dist_bgmm_edges_rows_dev).  Returns (edges,
    rows float32 [n_edges, 2], n_failed) as dist_edges_rows."""
    if model is None:
        raise ValueError("a prepared BGMM model is needed")
    return _fused_edges_rows("ppk_dist_bgmm_edges_rows_dev", ref, qry, kmers, random_tbl, random_correct, q_begin,
                             q_end, cap, C.byref(model))


def bgmm_edges_host(refs, qrys=None, kmers=None, random_tbl=None, model=None, random_correct=True, cap=None):
    """ppk_query_bgmm_edges_dbs: edges_host with the BGMM label test.  Returns (edges int64 [m,2] host, n_failed)."""
    if model is None:
        raise ValueError("a prepared BGMM model is needed")
    return _host_edges("ppk_query_bgmm_edges_dbs", refs, qrys, kmers, random_tbl, random_correct, cap,
                       C.byref(model))


def assign_threshold_dev(dist_t, slope, x_max, y_max, out=None):
    """poppunk_refine.assignThreshold on a resident float32 [n,2] CUDA tensor."""
    _check_dist_tensor(dist_t)
    n = dist_t.shape[0]
    if out is None:
        out = _torch().empty(n, dtype=_torch().float32, device=dist_t.device)
    _dev_call("ppk_assign_threshold_dev", dist_t.device, dist_t, n, int(slope), float(x_max), float(y_max), out)
    return out


def edge_threshold_dev(dist_t, slope, x_max, y_max, n_ref=0, inclusive=True, cap=None):
    """poppunk_refine.edgeThreshold on a resident float32 [n,2] CUDA tensor -> int64 [m,2]."""
    return _row_edges_dev("ppk_edge_threshold_dev", dist_t, cap, int(n_ref), int(slope), float(x_max), float(y_max),
                          1 if inclusive else 0)


def qc_edges_dev(dist_t, max_pi_dist, max_a_dist, n_ref=0, zero=False, cap=None):
    """qcDistMat's outlier edge lists on a resident float32 [n,2] CUDA tensor
    (PopPUNK/qc.py:332-337 long distances; :349-354 zero distances) -> int64 [m,2]."""
    return _row_edges_dev("ppk_qc_edges_dev", dist_t, cap, int(n_ref), 1 if zero else 0, float(max_pi_dist),
                          float(max_a_dist))


def _sweep_dev(launch, device, cap):
    """Run a boundary-sweep call, `launch(d_i, d_j, d_offset_idx, cap, d_n_out)`, with a capacity guess, once more
    with the exact size if the guess was short.  Returns the (i, j, offset_idx) int64 CUDA tensors."""
    torch = _torch()
    while True:
        buf = torch.empty((3, max(cap, 1)), dtype=torch.int64, device=device)
        n_out = torch.zeros(1, dtype=torch.int64, device=device)
        launch(buf[0], buf[1], buf[2], cap, n_out)
        m = int(n_out.item())
        if m <= cap:
            return buf[0, :m], buf[1, :m], buf[2, :m]
        cap = m


def threshold_iterate_1d_dev(dist_t, offsets, slope, x0, y0, x1, y1, cap=None):
    """poppunk_refine.thresholdIterate1D on a resident float32 [n,2] CUDA tensor ->
    (i, j, offset_idx) int64 CUDA tensors (src/boundary.cpp:154-210)."""
    off = np.ascontiguousarray(offsets, dtype=np.float64).ravel()
    n = dist_t.shape[0]
    return _sweep_dev(lambda i, j, o, c, n_out: _dev_call(
        "ppk_threshold_iterate_1d_dev", dist_t.device, dist_t, n, off, off.size, int(slope), float(x0), float(y0),
        float(x1), float(y1), i, j, o, c, n_out), dist_t.device, _cap_guess(n) if cap is None else cap)


def threshold_iterate_2d_dev(dist_t, x_max, y_max, cap=None):
    """poppunk_refine.thresholdIterate2D on a resident float32 [n,2] CUDA tensor ->
    (i, j, offset_idx) int64 CUDA tensors (src/boundary.cpp:212-237).  refine's 2-D mode calls it
    once per y value on the same matrix (PopPUNK/refine.py:587-593): resident, the 400 MB matrix is
    not re-sent for every y."""
    xm = np.ascontiguousarray(x_max, dtype=np.float32).ravel()
    if xm.size > 1 and np.any(np.diff(xm) < 0):
        raise RuntimeError("x_max range to thresholdIterate2D must be sorted")
    n = dist_t.shape[0]
    return _sweep_dev(lambda i, j, o, c, n_out: _dev_call(
        "ppk_threshold_iterate_2d_dev", dist_t.device, dist_t, n, xm, xm.size, float(y_max), i, j, o, c, n_out),
        dist_t.device, _cap_guess(n) if cap is None else cap)


def _edge_stream(i_t, j_t, off_t):
    """(m, stride) of the edge stream of network_sweep_dev / network_summary_dev, after checking its tensors."""
    torch = _torch()
    m = int(i_t.shape[0])
    for t in (i_t, j_t) + ((off_t,) if off_t is not None else ()):
        _check_tensor(t, "edge arrays must be int64 CUDA tensors of one length", torch.int64, (m,), contiguous=False)
    stride = i_t.stride(0) if m > 1 else 1
    if (m > 1 and j_t.stride(0) != stride) or stride not in (1, 2):
        raise TypeError("edge arrays must be contiguous, or the two columns of a contiguous [m, 2] tensor")
    if off_t is not None and off_t.stride(0) != 1 and m > 1:
        raise TypeError("the offset array must be contiguous")
    return m, stride


def network_sweep_dev(i_t, j_t, off_t, n, n_off, labels_at=None):
    """The counts behind networkSummary for every step of refine.growNetwork (ppk_network_sweep_dev):
    G_t = the edges (i_t[k], j_t[k]) with off_t[k] <= t over vertices 0 .. n-1.  int64 CUDA tensors of one length (a
    strided view such as edges[:, 0] is read in place); off_t None puts every edge at offset 0 (n_off must be 1).
    Returns (stats int64 [n_off, 4] = edges, components, triangles, connected triples; labels int32 [n] of
    G_{labels_at} numbered as scipy's connected_components, or None)."""
    torch = _torch()
    m, stride = _edge_stream(i_t, j_t, off_t)
    la = -1 if labels_at is None else int(labels_at)
    dev = i_t.device
    stats = torch.empty((max(int(n_off), 1), 4), dtype=torch.int64, device=dev)
    labels = torch.empty(max(int(n), 1), dtype=torch.int32, device=dev) if la >= 0 else None
    _dev_call("ppk_network_sweep_dev", dev, i_t, j_t, stride, off_t, m, int(n), int(n_off), la, stats, labels)
    return stats, (labels[:int(n)] if labels is not None else None)


_EDGES = "edges must be a contiguous int64 [m, 2] CUDA tensor"
_EDGES_OR_PAIR = _EDGES + ", or an (i, j) pair of int64 tensors"      # (what mst_dev and its kin have always said)


def _edge_cols(edges_t, message=_EDGES, pair=False):
    """(i_t, j_t): the two columns of a contiguous int64 [m, 2] CUDA edge list, read in place -- or, where the
    wrapper takes one (`pair`), the (i_t, j_t) pair itself, as network_sweep_dev takes it.  _edge_stream checks them."""
    if pair and isinstance(edges_t, (tuple, list)):
        return edges_t[0], edges_t[1]
    _check_tensor(edges_t, message, _torch().int64, (None, 2))
    return edges_t[:, 0], edges_t[:, 1]


def network_stats_dev(edges_t, n, labels=False):
    """network_sweep_dev of one int64 [m, 2] CUDA edge list (edge_threshold_dev, dist_edges, ...), read in place.
    Returns (stats int64 [4], labels int32 [n] or None)."""
    stats, lab = network_sweep_dev(*_edge_cols(edges_t), None, n, 1, 0 if labels else None)
    return stats[0], lab


def cluster_sweep_dev(i_t, j_t, off_t, n, n_off):
    """printClusters' cluster numbers of every vertex in every graph of a sweep (ppk_cluster_sweep_dev, DESIGN.md
    3.15): the edge stream of network_sweep_dev.  Returns (clusters int32 [n_off, n] CUDA: 1-based, by size descending,
    equal sizes by component index descending; n_clusters int32 [n_off] CUDA).  n_off == 1 with off_t None is the
    one-graph form."""
    torch = _torch()
    m, stride = _edge_stream(i_t, j_t, off_t)
    dev = i_t.device
    n, n_off = int(n), int(n_off)
    clusters = torch.empty((max(n_off, 1), max(n, 1)), dtype=torch.int32, device=dev)
    counts = torch.empty(max(n_off, 1), dtype=torch.int32, device=dev)
    if n != max(n, 1):                  # n == 0: a [n_off, 0] result over storage of its own
        clusters = clusters[:, :0]
    _dev_call("ppk_cluster_sweep_dev", dev, i_t, j_t, stride, off_t, m, n, n_off, clusters, counts)
    return clusters, counts


def cluster_numbers_dev(edges_t, n):
    """cluster_sweep_dev of one int64 [m, 2] CUDA edge list, read in place -> (numbers int32 [n] CUDA, the count)."""
    clusters, counts = cluster_sweep_dev(*_edge_cols(edges_t), None, n, 1)
    return clusters[0], int(counts[0].item())


def _assign_args(edges_t, ref_label_t):
    """(i_t, j_t, m, stride) of the query-vs-reference edge stream after checking it and the int32 label tensor.
    edges_t: a contiguous int64 [m, 2] CUDA tensor, or an (i_t, j_t) pair as network_sweep_dev takes it."""
    i_t, j_t = _edge_cols(edges_t, pair=True)
    m, stride = _edge_stream(i_t, j_t, None)
    _check_tensor(ref_label_t, "ref_label must be a contiguous int32 CUDA tensor on the edges' device",
                  _torch().int32, dim=1, like=i_t)
    return i_t, j_t, m, stride


def check_assign_sizes(who, n_ref, n_qry, max_links=None):
    """The size limits of ppk_query_links* / ppk_cluster_extend*, in the library's words, before any output is
    allocated (an n_qry of 2^31 would otherwise cost gigabytes just to be refused)."""
    if max_links is not None and not 1 <= max_links <= 64:
        raise RuntimeError("%s: max_links must be 1 .. 64" % who)
    if n_ref < 0 or n_qry < 0 or n_ref + n_qry >= 1 << 31:
        raise RuntimeError("%s: n_ref + n_qry must be < 2^31" % who)


def query_links_dev(edges_t, ref_label_t, n_qry, max_links=8):
    """Per query of a query-vs-reference edge stream (ppk_query_links_dev): vertices 0 .. n_ref-1 are
    references (n_ref = len(ref_label_t)), n_ref .. n_ref+n_qry-1 queries; ref_label_t int32 [n_ref] holds the component
    of every reference in the loaded network, any values in [0, n_ref).  Edges with both ends on one side are skipped.
    Returns CUDA tensors (degree int32 [n_qry]: query-reference edges; n_links int32 [n_qry]: distinct labels linked
    to, exact; links int32 [n_qry, max_links]: the smallest max_links of them, ascending, padded with -1)."""
    torch = _torch()
    i_t, j_t, m, stride = _assign_args(edges_t, ref_label_t)
    dev = i_t.device
    n_ref, n_qry, max_links = int(ref_label_t.shape[0]), int(n_qry), int(max_links)
    check_assign_sizes("ppk_query_links", n_ref, n_qry, max_links)
    degree = torch.empty(max(n_qry, 1), dtype=torch.int32, device=dev)
    n_links = torch.empty(max(n_qry, 1), dtype=torch.int32, device=dev)
    links = torch.empty((max(n_qry, 1), max_links), dtype=torch.int32, device=dev)
    _dev_call("ppk_query_links_dev", dev, i_t, j_t, stride, m, ref_label_t, n_ref, n_qry, max_links, degree, n_links,
              links)
    return degree[:n_qry], n_links[:n_qry], links[:n_qry]


def cluster_extend_dev(edges_t, ref_label_t, n_qry):
    """printClusters' number of every vertex of (the loaded network + these edges), the loaded network given by its
    component labels alone (ppk_cluster_extend_dev): what cluster_numbers_dev gives on the union of
    the reference network's edges and edges_t, without reading the former.  The stream and labels of
    query_links_dev; query-query and reference-reference edges take part.  Returns (numbers int32 [n_ref + n_qry]
    CUDA, the cluster count)."""
    torch = _torch()
    i_t, j_t, m, stride = _assign_args(edges_t, ref_label_t)
    dev = i_t.device
    n_ref, n_qry = int(ref_label_t.shape[0]), int(n_qry)
    check_assign_sizes("ppk_cluster_extend", n_ref, n_qry)
    numbers = torch.empty(max(n_ref + n_qry, 1), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _dev_call("ppk_cluster_extend_dev", dev, i_t, j_t, stride, m, ref_label_t, n_ref, n_qry, numbers, count)
    return numbers[:n_ref + n_qry], int(count.item())


REFS_COUNT_NAMES = ("references", "reference_edges", "components", "cliques_removed", "from_cliques", "from_small",
                    "added_by_repair", "components_repaired")


def pick_references_dev(edges_t, n, existing=None, merged=None, fast=False):
    """extractReferences' choice of reference genomes as the deterministic rule of DESIGN.md 3.25
    (ppk_pick_refs_dev): clique pruning per component (fast: fastPrune's rank test), then the repair that joins the
    references of a component.  edges_t: a contiguous int64 [m, 2] CUDA tensor or an (i_t, j_t) pair, read in place;
    existing, merged: uint8 / bool CUDA tensors of n flags, or None.  Returns (is_ref uint8 [n] CUDA, ref_edges int64
    [k, 2] CUDA: the edges among references in stream order, renumbered by rank, counts: a dict of REFS_COUNT_NAMES)."""
    torch = _torch()
    i_t, j_t = _edge_cols(edges_t, pair=True)
    m, stride = _edge_stream(i_t, j_t, None)
    dev = i_t.device
    n = int(n)
    if n < 0 or n >= 1 << 31:
        raise RuntimeError("ppk_pick_refs: n_vertices must be < 2^31")
    flags = []
    for name, f in (("existing", existing), ("merged", merged)):
        if f is not None:
            _check_tensor(f, "%s must be a uint8 or bool CUDA tensor of n flags on the edges' device" % name,
                          (torch.uint8, torch.bool), (n,), like=i_t, contiguous=False)
            f = f.contiguous().view(torch.uint8)
        flags.append(f)
    is_ref = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    ref_edges = torch.empty((max(m, 1), 2), dtype=torch.int64, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    _dev_call("ppk_pick_refs_dev", dev, i_t, j_t, stride, m, n, flags[0], flags[1], 1 if fast else 0, is_ref,
              ref_edges, counts)
    c = dict(zip(REFS_COUNT_NAMES, counts.cpu().tolist()))
    return is_ref[:n], ref_edges[:c["reference_edges"]], c


def pick_references(edges, n, existing=None, merged=None, fast=False, device=0):
    """pick_references_dev on host arrays (ppk_pick_refs): edges int64 [m, 2], existing / merged n flags or None ->
    (is_ref uint8 [n], ref_edges int64 [k, 2], counts dict)."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    i, j = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    n, m = int(n), e.shape[0]
    if n < 0 or n >= 1 << 31:
        raise RuntimeError("ppk_pick_refs: n_vertices must be < 2^31")
    flags = []
    for name, f in (("existing", existing), ("merged", merged)):
        if f is not None:
            f = np.ascontiguousarray(np.asarray(f) != 0, dtype=np.uint8).ravel()
            if f.size != n:
                raise ValueError("%s must hold n flags" % name)
        flags.append(f)
    is_ref = np.zeros(max(n, 1), dtype=np.uint8)
    ref_edges = np.zeros((max(m, 1), 2), dtype=np.int64)
    counts = np.zeros(8, dtype=np.int64)
    _lib.call("ppk_pick_refs", i, j, m, n, flags[0], flags[1], 1 if fast else 0, int(device), is_ref, ref_edges,
              counts)
    c = dict(zip(REFS_COUNT_NAMES, counts.tolist()))
    return is_ref[:n], ref_edges[:c["reference_edges"]], c


def nearest_reference_dev(dist_t, n_qry, n_ref, dist_col=0):
    """get_kNN_distances(qrDistMat[:, dist_col].reshape(n_qry, n_ref), kNN=1) as assign_query_hdf5's `stable` branch
    calls it (PopPUNK/assign.py:678-684), on the resident float32 [n_qry * n_ref, 2] matrix, read in place
    (ppk_knn_rect_dev): for every query the reference of the smallest distance, ties by the lower index -- and, as
    upstream, never the reference whose INDEX equals the query's (src/extend.cpp:271 skips column i of row i, also in
    a rectangle).  Returns int64 [n_qry] CUDA."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    n_qry, n_ref = int(n_qry), int(n_ref)
    if dist_t.shape[0] != n_qry * n_ref:
        raise ValueError("the matrix must have n_qry * n_ref rows")
    dev = dist_t.device
    oi = torch.empty(max(n_qry, 1), dtype=torch.int64, device=dev)
    oj = torch.zeros(max(n_qry, 1), dtype=torch.int64, device=dev)
    od = torch.empty(max(n_qry, 1), dtype=torch.float32, device=dev)
    if n_qry and n_ref:
        _dev_call("ppk_knn_rect_dev", dev, dist_t, 2, int(dist_col), n_qry, n_ref, 0, 1, oi, oj, od)
    return oj[:n_qry]


def pair_sum_shift(n_rows):
    """The fixed-point shift of cluster_pair_sums: min(40, 62 - ceil_log2(n_rows)), so that no sum passes 2^62
    (ceil_log2 as ppk_device.h states it)."""
    r = 0
    while r < 62 and (1 << r) < int(n_rows):
        r += 1
    return min(40, 62 - r)


def cluster_pair_sums_dev(dist_t, levels_t, col=0, shift=None):
    """One pass over a resident float32 [n(n-1)/2, 2] CUDA matrix (ppk_cluster_pair_sums_dev):
    levels_t int32 [n_levels, n] CUDA, nested cluster numbers in [1, n].  Every row (i, j) adds
    llrint(dist[row, col] * 2^shift) to bucket (t*, c): the first level at which i and j share a cluster, and that
    cluster.  Returns (sum, cnt) int64 [n_levels, n + 1] CUDA and the shift.  Nesting is the caller's precondition
    (iterate.check_nested)."""
    torch = _torch()
    n_rows, n, n_levels = _condensed_and_levels(dist_t, levels_t)
    if shift is None:
        shift = pair_sum_shift(n_rows)
    out = torch.empty((2, max(n_levels, 1), n + 1), dtype=torch.int64, device=dist_t.device)
    _dev_call("ppk_cluster_pair_sums_dev", dist_t.device, dist_t, n_rows, int(col), levels_t, n_levels, int(shift),
              out[0], out[1])
    return out[0], out[1], int(shift)


def _condensed_and_levels(dist_t, levels_t):
    """(rows, samples, levels) of a resident condensed [n(n-1)/2, 2] matrix and the int32 [n_levels, n] cluster
    numbers that go with it, after checking both."""
    _check_dist_tensor(dist_t)
    n_rows = int(dist_t.shape[0])
    n = _samples_of(n_rows)
    _check_tensor(levels_t, "levels must be a contiguous int32 [n_levels, %d] CUDA tensor on the matrix's device" % n,
                  _torch().int32, (None, n), like=dist_t)
    return n_rows, n, int(levels_t.shape[0])


def silhouette_shift(n):
    """The fixed-point shift of the silhouette's sums: min(40, 61 - ceil_log2(n)), so that no sum of n distances of at
    most sqrt 2 passes 2^62 (ceil_log2 as ppk_device.h states it)."""
    r = 0
    while r < 62 and (1 << r) < int(n):
        r += 1
    return min(40, 61 - r)


def silhouette_dev(dist_t, levels_t, metric=2, shift=None, want_ab=False):
    """The silhouette of every sample under every level (ppk_silhouette_dev, DESIGN.md 3.19;
    tests/silhouette_model.py restates the rule): dist_t a resident float32 [n(n-1)/2, 2] CUDA matrix, levels_t int32
    [n_levels, n] CUDA, cluster numbers in [1, n] (gaps allowed, levels need not be nested).  metric: 0 core,
    1 accessory, 2 euclidean, 3 difference.  Returns (s float64 [n_levels, n], n_labels int32 [n_levels], valid int32
    [n_levels]) as CUDA tensors -- the rows of an invalid level (fewer than 2 or more than n - 1 labels) are NaN -- and
    with want_ab the mean distances (a, b) float64 [n_levels, n] as a fourth and fifth item."""
    torch = _torch()
    n_rows, n, n_levels = _condensed_and_levels(dist_t, levels_t)
    if shift is None:
        shift = silhouette_shift(n)
    dev = dist_t.device
    out = torch.empty((3 if want_ab else 1, max(n_levels, 1), n), dtype=torch.float64, device=dev)
    counts = torch.empty((2, max(n_levels, 1)), dtype=torch.int32, device=dev)
    _dev_call("ppk_silhouette_dev", dev, dist_t, n_rows, int(metric), levels_t, n_levels, int(shift),
              out[1] if want_ab else None, out[2] if want_ab else None, out[0], counts[0], counts[1])
    if want_ab:
        return out[0], counts[0], counts[1], out[1], out[2]
    return out[0], counts[0], counts[1]


def contingency_sums_dev(levels_a, levels_b=None):
    """The integer sums the Rand and adjusted Rand indices are made of (ppk_contingency_sums_dev, DESIGN.md 3.20;
    tests/contingency_model.py restates them): levels_a int32 [n_a, n] CUDA, levels_b int32 [n_b, n] CUDA or None for
    B = A, cluster numbers in [1, n] (gaps allowed, levels need not be nested; engine.cluster_sweep_dev's rows
    qualify).  Returns (sq_a int64 [n_a], sq_b int64 [n_b], labels_a int32 [n_a], labels_b int32 [n_b], sq_cells int64
    [n_a, n_b], n_cells int64 [n_a, n_b]) as CUDA tensors: the squared class sizes and the label count of every level,
    the squared cell sizes and the non-empty cells of every pair's contingency table."""
    torch = _torch()

    def check(t, what):
        _check_tensor(t, "%s must be a contiguous int32 [n_levels, n] CUDA tensor" % what, torch.int32, dim=2)

    check(levels_a, "levels_a")
    n_a, n = int(levels_a.shape[0]), int(levels_a.shape[1])
    n_b = n_a
    if levels_b is not None:
        check(levels_b, "levels_b")
        if int(levels_b.shape[1]) != n or levels_b.device != levels_a.device:
            raise TypeError("levels_b must have levels_a's %d samples and live on its device" % n)
        n_b = int(levels_b.shape[0])
    dev = levels_a.device
    sq = [torch.empty(max(k, 1), dtype=torch.int64, device=dev) for k in (n_a, n_b)]
    labels = [torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (n_a, n_b)]
    cells = torch.empty((2, max(n_a, 1), max(n_b, 1)), dtype=torch.int64, device=dev)
    _dev_call("ppk_contingency_sums_dev", dev, levels_a, n_a, levels_b, n_b, n, sq[0], sq[1], labels[0], labels[1],
              cells[0], cells[1])
    return sq[0][:n_a], sq[1][:n_b], labels[0][:n_a], labels[1][:n_b], cells[0][:n_a, :n_b], cells[1][:n_a, :n_b]


def sketch_dev(codes_t, seq_off, kmers, sketchsize64, bbits=14, strand_preserved=False):
    """Bin sketches of the samples in codes_t (ppk_sketch_dev; tests/sketch_model.py restates the
    rule): codes_t uint8 CUDA (0-3 = A, C, G, T; 4 = any other residue; 5 = contig break), seq_off the n + 1 offsets
    of the samples in it (host array or int64 CUDA tensor), kmers the k-mer lengths (host).  Returns CUDA tensors
    (sketches int64 [n, nk, sketchsize64 * bbits] ready for SketchDB, stats int64 [n, 6] = length, missing bases,
    A, C, G, T counts, filled int32 [n, nk] = non-empty bins before empty ones were filled).  [EXT] The rule is this
    project's own: sketches made here do not match those of pp-sketchlib."""
    torch = _torch()
    dev, off_t, n, k, nk, words = _sketch_args(codes_t, seq_off, kmers, sketchsize64, bbits)
    sketches = torch.zeros((n, nk, max(words, 0)), dtype=torch.int64, device=dev)
    stats = torch.zeros((n, 6), dtype=torch.int64, device=dev)
    filled = torch.zeros((n, nk), dtype=torch.int32, device=dev)
    # an empty tensor has address 0 and NULL is an error to the library: it gets the offsets' address (never used)
    _dev_call("ppk_sketch_dev", dev, C.c_void_p(codes_t.data_ptr() if codes_t.numel() else off_t.data_ptr()), off_t,
              n, k, nk, int(sketchsize64), int(bbits), _lib.SKETCH_STRAND_PRESERVED if strand_preserved else 0,
              C.c_void_p(sketches.data_ptr() or off_t.data_ptr()), C.c_void_p(stats.data_ptr() or off_t.data_ptr()),
              C.c_void_p(filled.data_ptr() or off_t.data_ptr()))
    return sketches, stats, filled


def _sketch_args(codes_t, seq_off, kmers, sketchsize64, bbits):
    """(device, offsets int64 CUDA [n + 1], n, k-mer lengths int32, nk, words a sketch) of the two sketch calls, after
    checking the codes and the offsets."""
    torch = _torch()
    _check_tensor(codes_t, "codes_t must be a contiguous one-dimensional uint8 CUDA tensor", torch.uint8, dim=1)
    dev = codes_t.device
    if hasattr(seq_off, "is_cuda"):
        off_t = seq_off.to(device=dev, dtype=torch.int64).contiguous()
    else:
        off_t = torch.as_tensor(np.ascontiguousarray(seq_off, dtype=np.int64), device=dev)
    if off_t.dim() != 1 or off_t.numel() < 1:
        raise ValueError("seq_off must be a one-dimensional array of n + 1 offsets")
    n = int(off_t.numel()) - 1
    if n > 0 and not hasattr(seq_off, "is_cuda") and int(np.asarray(seq_off).ravel()[-1]) > int(codes_t.numel()):
        raise ValueError("seq_off ends beyond codes_t")
    k = np.ascontiguousarray(kmers, dtype=np.int32).ravel()
    return dev, off_t, n, k, int(k.size), int(sketchsize64) * int(bbits)


def sketch_reads_dev(codes_t, seq_off, kmers, sketchsize64, min_count, exact=False, bbits=14, strand_preserved=False):
    """Bin sketches of the read samples in codes_t (ppk_sketch_reads_dev; tests/sketch_reads_model.py
    restates the rule): as sketch_dev, every read a contig (a code 5 between reads), with a k-mer entering a bin only
    when the sample holds it at least min_count times (exact: the exact route; otherwise the count table [EXT]).
    Returns CUDA tensors (sketches, stats, filled, kstats int64 [n, nk, 4] = occ, adm_occ, filled, win_occ);
    stats[:, 0] is the estimate of the distinct admitted k-mers at the largest k."""
    torch = _torch()
    dev, off_t, n, k, nk, words = _sketch_args(codes_t, seq_off, kmers, sketchsize64, bbits)
    flags = (_lib.SKETCH_STRAND_PRESERVED if strand_preserved else 0) | (_lib.SKETCH_EXACT if exact else 0)
    sketches = torch.zeros((n, nk, max(words, 0)), dtype=torch.int64, device=dev)
    stats = torch.zeros((n, 6), dtype=torch.int64, device=dev)
    kstats = torch.zeros((n, nk, 4), dtype=torch.int64, device=dev)
    filled = torch.zeros((n, nk), dtype=torch.int32, device=dev)
    # (empty tensors: the offsets' address, as sketch_dev)
    _dev_call("ppk_sketch_reads_dev", dev, C.c_void_p(codes_t.data_ptr() if codes_t.numel() else off_t.data_ptr()),
              off_t, n, k, nk, int(sketchsize64), int(bbits), flags, int(min_count),
              C.c_void_p(sketches.data_ptr() or off_t.data_ptr()), C.c_void_p(stats.data_ptr() or off_t.data_ptr()),
              C.c_void_p(kstats.data_ptr() or off_t.data_ptr()), C.c_void_p(filled.data_ptr() or off_t.data_ptr()))
    return sketches, stats, filled, kstats


def _strain_segments(seg_off):
    seg = np.ascontiguousarray(seg_off, dtype=np.int64)
    if seg.ndim != 1 or seg.shape[0] < 2:
        raise ValueError("seg_off must be a one-dimensional array of n_strains + 1 offsets")
    return seg


def strain_nnz(seg_off, depth):
    """The entries of strain_knn_dev's lists: the sum over the strains of n_s * min(depth, n_s - 1)."""
    sizes = np.diff(_strain_segments(seg_off))
    return int((sizes * np.minimum(int(depth), sizes - 1)).sum())


def strain_knn_dev(dist_t, members_t, seg_off, depth, dist_col=0):
    """Every member's min(depth, n_s - 1) nearest members of its own strain, for all strains in one call
    (ppk_strain_knn_dev; tests/lineage_model.py restates it): dist_t the resident float32
    [n(n-1)/2, 2] CUDA matrix, members_t int64 [m] CUDA (the strains' member lists back to back, global ids, each in
    the strain's local order), seg_off the n_strains + 1 offsets (host).  Returns CUDA tensors (i, j, dist) with LOCAL
    indices, strain by strain and row by row: per strain what ppk_knn_dev gives on its pruned square."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    n_rows = int(dist_t.shape[0])
    n = _samples_of(n_rows)
    if n * (n - 1) // 2 != n_rows:
        raise ValueError("the matrix must hold n(n-1)/2 rows")
    _check_tensor(members_t, "members must be a contiguous int64 [m] CUDA tensor on the matrix's device", torch.int64,
                  dim=1, like=dist_t)
    seg = _strain_segments(seg_off)
    if int(seg[-1]) != int(members_t.shape[0]):
        raise ValueError("seg_off must end at the number of members")
    sizes = np.diff(seg)
    nnz = strain_nnz(seg, depth) if len(sizes) and sizes.min() >= 2 and int(depth) >= 1 else 0
    oi, oj, od = _neighbour_outputs(max(nnz, 1), dist_t.device)
    _dev_call("ppk_strain_knn_dev", dist_t.device, dist_t, n, int(dist_col), members_t, seg, len(seg) - 1, int(depth),
              oi, oj, od)
    return oi[:nnz], oj[:nnz], od[:nnz]


def qr_row_index(q, r, n_ref):
    """The row of pair (query q, reference r) in the query-major [n_qry * n_ref, 2] matrix, as the kernels of
    strain_extend_dev compute it: 64-bit, q * n_ref + r passes 2^31 on large databases."""
    return int(np.int64(q) * np.int64(n_ref) + np.int64(r))


def strain_extend_dev(members_t, seg_off, queries_t, qry_off, nn_j_t, nn_d_t, qr_t, qq_t, n_ref, n_qry, depth,
                      dist_col=0, floor=1e-10):
    """poppunk_refine.extend inside every strain in one call (ppk_strain_extend_dev, DESIGN.md 3.22;
    tests/strain_extend_model.py restates it): members_t / seg_off as strain_knn_dev takes them; queries_t int64 [mq]
    CUDA with qry_off (host), the query ids of every strain back to back (a strain may have none); nn_j_t / nn_d_t the
    stored lists in strain_knn_dev's layout for (seg_off, depth); qr_t the resident float32 [n_qry * n_ref, 2]
    query-major matrix; qq_t the float32 [n_qry(n_qry-1)/2, 2] long form of the queries, or None when no strain has
    two.  Returns CUDA tensors (i, j, dist) with LOCAL indices over the n_s + q_s rows of every strain (members, then
    queries), min(depth, n_s + q_s - 1) entries a row: strain_knn_dev's layout for seg_off + qry_off, which is what
    strain_ranks_dev takes."""
    torch = _torch()
    dev = members_t.device

    for t, dtype in ((members_t, torch.int64), (nn_j_t, torch.int64), (nn_d_t, torch.float32)):
        _check_tensor(t, "members, and the stored lists, must be contiguous CUDA tensors on one device: int64 [m], "
                      "int64 and float32 [nnz]", dtype, dim=1, like=members_t)
    seg, qoff = _strain_segments(seg_off), _strain_segments(qry_off)
    if seg.shape != qoff.shape:
        raise ValueError("seg_off and qry_off must have one entry per strain and one more")
    if int(seg[-1]) != int(members_t.shape[0]):
        raise ValueError("seg_off must end at the number of members")
    mq = int(qoff[-1])
    if mq:
        _check_tensor(queries_t, "queries must be a contiguous int64 [mq] CUDA tensor on the members' device, qry_off "
                      "ending at mq", torch.int64, (mq,), like=members_t)
        _check_tensor(qr_t, "qr must be a contiguous float32 [n_qry * n_ref, 2] CUDA tensor on the members' device",
                      torch.float32, (int(n_qry) * int(n_ref), 2), like=members_t)
    if qq_t is not None:
        _check_tensor(qq_t, "qq must be a contiguous float32 [n_qry(n_qry-1)/2, 2] CUDA tensor on the members' device",
                      torch.float32, (int(n_qry) * (int(n_qry) - 1) // 2, 2), like=members_t)
    sizes = np.diff(seg)
    valid = len(sizes) and sizes.min() >= 2 and int(depth) >= 1 and np.diff(qoff).min() >= 0
    if valid and strain_nnz(seg, depth) != int(nn_j_t.shape[0]) or nn_j_t.shape != nn_d_t.shape:
        raise ValueError("the stored lists must hold the entries of strain_knn_dev at this depth")
    nnz = strain_nnz(seg + qoff, depth) if valid else 0
    oi, oj, od = _neighbour_outputs(max(nnz, 1), dev)
    _dev_call("ppk_strain_extend_dev", dev, members_t, seg, queries_t if mq else None, qoff, len(seg) - 1, nn_j_t,
              nn_d_t, qr_t if mq else None, qq_t, int(n_ref), int(n_qry), int(dist_col), float(np.float32(floor)),
              int(depth), oi, oj, od)
    return oi[:nnz], oj[:nnz], od[:nnz]


def strain_ranks_dev(j_t, d_t, seg_off, depth, ranks, reciprocal_only=False, count_unique_distances=False,
                     epsilon=1e-10):
    """lowerRank's rule for every rank on strain_knn_dev's sorted lists (ppk_strain_ranks_dev): j_t,
    d_t the lists, same seg_off and depth, ranks ascending.  Returns (prefix int32 [n_ranks, m]: the entries of each
    row each rank keeps; pos_i, pos_j, level int64 and dist float32: the level stream, positions into the member
    array, every unordered pair once -- an edge stream for cluster_sweep_dev with n = m, n_off = n_ranks)."""
    torch = _torch()
    for t, dtype, shape in ((j_t, torch.int64, (None,)), (d_t, torch.float32, tuple(j_t.shape))):
        _check_tensor(t, "the lists must be contiguous CUDA tensors of one length, int64 columns and float32 "
                      "distances", dtype, shape, like=j_t)
    seg = _strain_segments(seg_off)
    rk = np.ascontiguousarray(ranks, dtype=np.int32)
    if rk.ndim != 1 or rk.shape[0] < 1:
        raise ValueError("ranks must be a non-empty one-dimensional array")
    m, n_ranks = int(seg[-1]), int(rk.shape[0])
    sizes = np.diff(seg)
    ok = len(sizes) and sizes.min() >= 2 and int(depth) >= 1
    nnz = strain_nnz(seg, depth) if ok else 0
    if ok and nnz != int(j_t.shape[0]):
        raise ValueError("the lists must hold the %d entries of strain_knn_dev at this depth" % nnz)
    # the stream holds no more than the last rank's prefixes: known exactly without count_unique_distances
    cap = nnz if count_unique_distances or not ok else int((sizes * np.minimum(
        np.minimum(int(depth), sizes - 1), int(rk.max()) + 1)).sum())
    dev = j_t.device
    prefix = torch.empty((n_ranks, max(m, 1)), dtype=torch.int32, device=dev)
    pos = torch.empty((3, max(cap, 1)), dtype=torch.int64, device=dev)
    sd = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    n_out = C.c_size_t(0)
    _dev_call("ppk_strain_ranks_dev", dev, j_t, d_t, seg, len(seg) - 1, int(depth), rk, n_ranks,
              int(bool(reciprocal_only)), int(bool(count_unique_distances)), float(np.float32(epsilon)), prefix,
              pos[0], pos[1], pos[2], sd, cap, C.byref(n_out))
    k = int(n_out.value)
    return prefix[:, :m], pos[0, :k], pos[1, :k], pos[2, :k], sd[:k]


def strain_cluster_numbers(clusters_t, seg_off):
    """cluster_sweep_dev's rows over the m positions of all strains -> every strain's own printClusters numbers: a
    member's number is the dense rank of its number among the numbers of its segment (positions keep local order
    inside a segment, and components are ranked by size, then by their first vertex)."""
    torch = _torch()
    seg = _strain_segments(seg_off)
    m = int(seg[-1])
    seg_id = torch.as_tensor(np.repeat(np.arange(len(seg) - 1, dtype=np.int64), np.diff(seg)), device=clusters_t.device)
    out = torch.empty_like(clusters_t)
    for t in range(int(clusters_t.shape[0])):
        key = seg_id * (m + 1) + clusters_t[t].to(torch.int64)
        _, inverse = torch.unique(key, sorted=True, return_inverse=True)
        first = torch.full((len(seg) - 1,), m, dtype=torch.int64, device=clusters_t.device)
        first.scatter_reduce_(0, seg_id, inverse, reduce="amin")
        out[t] = (inverse - first[seg_id] + 1).to(torch.int32)
    return out


def _kde_args(gx, gy, scale):
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    gy = np.ascontiguousarray(gy, dtype=np.float64)
    if gx.ndim != 1 or gy.ndim != 1:
        raise ValueError("gx and gy must be one-dimensional")
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32).reshape(2)
    return gx, gy, sc


def density_kde_dev(dist_t, gx, gy, h, scale=None, idx_t=None, shift=None, return_scale=False):
    """The Epanechnikov sums of a resident float32 [n, 2] CUDA matrix on the nodes (gx[a], gy[b])
    (ppk_density_kde_dev; tests/density_model.py restates the rule).  gx, gy: ascending float64 host
    arrays; h: the bandwidth; scale: two float32, or None for the column maxima of the rows read, taken on the device
    (np.amax(X, axis=0)); idx_t: an int64 CUDA index list (any order, repeats allowed), or None for every row; shift:
    None = pair_sum_shift(rows read).  Returns (sum int64 [nx, ny] CUDA, shift, rows_read), and with return_scale the
    float32 [2] the call divided by as a fourth item.  sklearn's density is sum * 2^-shift * 2 / (pi h^2 N)."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    gx, gy, sc = _kde_args(gx, gy, scale)
    n_rows = int(dist_t.shape[0])
    if idx_t is not None:
        _check_tensor(idx_t, "idx must be a contiguous int64 CUDA vector on the matrix's device", torch.int64, dim=1,
                      like=dist_t)
    rows_read = n_rows if idx_t is None else int(idx_t.shape[0])
    if shift is None:
        shift = pair_sum_shift(rows_read)
    used = np.zeros(2, dtype=np.float32)
    # NULL means every row, and an empty tensor has no address: an empty list passes the matrix's (never read)
    idx_p = None if idx_t is None else C.c_void_p(idx_t.data_ptr() or dist_t.data_ptr())
    out = torch.empty((len(gx), len(gy)), dtype=torch.int64, device=dist_t.device)
    _dev_call("ppk_density_kde_dev", dist_t.device, dist_t, n_rows, idx_p, rows_read if idx_t is not None else 0, sc,
              gx, len(gx), gy, len(gy), float(h), int(shift), out, used)
    return (out, int(shift), rows_read, used) if return_scale else (out, int(shift), rows_read)


def density_kde(dist, gx, gy, h, scale=None, idx=None, shift=None, device=0):
    """density_kde_dev for host arrays (ppk_density_kde): dist float32 [n, 2], idx int64 or None.  Returns (sum int64
    [nx, ny] numpy, shift, rows_read, scale float32 [2])."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    if dist.ndim != 2 or dist.shape[1] != 2:
        raise ValueError("dist must be [n, 2]")
    gx, gy, sc = _kde_args(gx, gy, scale)
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).ravel()
    rows_read = dist.shape[0] if ix is None else len(ix)
    if shift is None:
        shift = pair_sum_shift(rows_read)
    out = np.empty((len(gx), len(gy)), dtype=np.int64)
    used = np.zeros(2, dtype=np.float32)
    _lib.call("ppk_density_kde", dist, dist.shape[0], ix, rows_read if ix is not None else 0, sc, gx, len(gx), gy,
              len(gy), float(h), int(shift), int(device), out, used)
    return out, int(shift), rows_read, used


def _raster_args(raster):
    x0, inv_dx, nx, y0, inv_dy, ny = raster
    return float(x0), float(inv_dx), int(nx), float(y0), float(inv_dy), int(ny)


def density_counts_dev(dist_t, raster, labels_t=None, label_lo=0, n_slots=1):
    """Which pixels of a uniform raster hold a row, per label (ppk_density_counts_dev).  raster =
    (x0, inv_dx, nx, y0, inv_dy, ny); a row (x, y) falls in pixel (floor((x - x0) * inv_dx), floor((y - y0) * inv_dy))
    of slot labels[row] - label_lo (no labels: slot 0).  labels_t: the int32 [n] CUDA tensor bgmm_assign_dev or
    dbscan_assign_dev returns.  Returns (counts uint32 [n_slots, ny, nx] CUDA, outside int64 [1] CUDA: the rows off
    the raster)."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    x0, inv_dx, nx, y0, inv_dy, ny = _raster_args(raster)
    n_rows = int(dist_t.shape[0])
    if labels_t is not None:
        _check_tensor(labels_t, "labels must be a contiguous int32 [n] CUDA tensor on the matrix's device",
                      torch.int32, (n_rows,), like=dist_t)
    if not (1 <= int(n_slots) <= 32 and 1 <= nx <= 4096 and 1 <= ny <= 4096):
        raise ValueError("n_slots must be 1 .. 32 and nx, ny 1 .. 4096")
    dev = dist_t.device
    counts = torch.empty((int(n_slots), ny, nx), dtype=torch.uint32, device=dev)
    outside = torch.empty(1, dtype=torch.int64, device=dev)
    _dev_call("ppk_density_counts_dev", dev, dist_t, n_rows, labels_t, int(label_lo), int(n_slots), x0, inv_dx, nx, y0,
              inv_dy, ny, counts, outside)
    return counts, outside


def density_counts(dist, raster, labels=None, label_lo=0, n_slots=1, device=0):
    """density_counts_dev for host arrays (ppk_density_counts).  Returns (counts uint32 [n_slots, ny, nx] numpy, the
    number of rows off the raster)."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    if dist.ndim != 2 or dist.shape[1] != 2:
        raise ValueError("dist must be [n, 2]")
    x0, inv_dx, nx, y0, inv_dy, ny = _raster_args(raster)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32).ravel()
    if lab is not None and len(lab) != dist.shape[0]:
        raise ValueError("one label per row")
    if not (1 <= int(n_slots) <= 32 and 1 <= nx <= 4096 and 1 <= ny <= 4096):
        raise ValueError("n_slots must be 1 .. 32 and nx, ny 1 .. 4096")
    counts = np.empty((int(n_slots), ny, nx), dtype=np.uint32)
    outside = np.zeros(1, dtype=np.int64)
    _lib.call("ppk_density_counts", dist, dist.shape[0], lab, int(label_lo), int(n_slots), x0, inv_dx, nx, y0, inv_dy,
              ny, int(device), counts, outside)
    return counts, int(outside[0])


def network_summary_dev(i_t, j_t, off_t, n, n_off, values_at=None):
    """network_sweep_dev plus networkSummary's betweenness for every G_t (ppk_network_summary_dev).
    The same edge stream and checks.  Returns (stats int64 [n_off, 4], bit for bit network_sweep_dev's; bt float64
    [n_off, 2] = mean and size-weighted mean over the components of more than 3 vertices of their maximum normalised
    vertex betweenness; scored int64 [n_off] = how many such components; values float64 [n] = every vertex's
    normalised betweenness in G_{values_at} within its component, or None), CUDA tensors."""
    return _network_summary("ppk_network_summary_dev", i_t, j_t, off_t, n, n_off, values_at)


def _network_summary(name, i_t, j_t, off_t, n, n_off, values_at, *sampling):
    """The body of network_summary_dev and network_summary_sampled_dev: the latter's call ends in `sampling`."""
    torch = _torch()
    m, stride = _edge_stream(i_t, j_t, off_t)
    va = -1 if values_at is None else int(values_at)
    dev = i_t.device
    no = max(int(n_off), 1)
    stats = torch.empty((no, 4), dtype=torch.int64, device=dev)
    bt = torch.empty((no, 2), dtype=torch.float64, device=dev)
    scored = torch.empty(no, dtype=torch.int64, device=dev)
    values = torch.empty(max(int(n), 1), dtype=torch.float64, device=dev) if va >= 0 else None
    _dev_call(name, dev, i_t, j_t, stride, off_t, m, int(n), int(n_off), va, stats, bt, scored, values, *sampling)
    return stats, bt, scored, (values[:int(n)] if values is not None else None)


def network_summary_graph_dev(edges_t, n, values=False):
    """network_summary_dev of one int64 [m, 2] CUDA edge list, read in place.  Returns (stats int64 [4], bt float64
    [2], scored int64 [] and values float64 [n] or None)."""
    stats, bt, scored, val = network_summary_dev(*_edge_cols(edges_t), None, n, 1, 0 if values else None)
    return stats[0], bt[0], scored[0], val


def network_summary_sampled_dev(i_t, j_t, off_t, n, n_off, values_at=None, sources=100, seed=0, whole_graph=False):
    """network_summary_dev from at most `sources` Brandes sources per component, the sample fixed by `seed`
    (ppk_network_summary_sampled_dev): components of at most `sources` vertices give
    network_summary_dev's bits.  whole_graph: `values` are vertex_betweenness(G, norm=True) of the whole graph
    (components of 3 vertices included, divisor (n - 1)(n - 2)); bt and scored do not change.  Same returns."""
    sources = int(sources)
    if sources < 1:
        raise ValueError("network_summary_sampled_dev: sources must be >= 1")
    return _network_summary("ppk_network_summary_sampled_dev", i_t, j_t, off_t, n, n_off, values_at, sources,
                            int(seed) & ((1 << 64) - 1), _lib.BT_WHOLE_GRAPH if whole_graph else 0)


def network_summary_sampled_graph_dev(edges_t, n, values=False, sources=100, seed=0, whole_graph=False):
    """network_summary_sampled_dev of one int64 [m, 2] CUDA edge list, read in place; network_summary_graph_dev's
    returns."""
    stats, bt, scored, val = network_summary_sampled_dev(*_edge_cols(edges_t), None, n, 1, 0 if values else None,
                                                         sources, seed, whole_graph)
    return stats[0], bt[0], scored[0], val


def mst_dev(edges_t, w_t, n, labels=False):
    """The minimum spanning forest of a weighted multigraph (ppk_mst_dev).  edges_t: an int64 [m, 2]
    CUDA tensor or (i_t, j_t) as network_sweep_dev takes them; w_t: float32 [m] CUDA weights.  Edges are totally
    ordered by (w, min, max, index), so the forest is unique.  Returns (tree_idx int64 [n - components]: the input
    indices of the forest's edges, ascending; the number of components; labels int32 [n] numbered as scipy's
    connected_components numbers them, or None), CUDA tensors and an int."""
    torch = _torch()
    i_t, j_t = _edge_cols(edges_t, _EDGES_OR_PAIR, pair=True)
    m, stride = _edge_stream(i_t, j_t, None)
    _check_tensor(w_t, "weights must be a contiguous float32 CUDA tensor, one per edge", torch.float32, (m,))
    n = int(n)
    dev = i_t.device
    tree = torch.empty(max(min(m, n - 1), 1), dtype=torch.int64, device=dev)
    n_tree = torch.zeros(1, dtype=torch.int64, device=dev)
    lab = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if labels else None
    _dev_call("ppk_mst_dev", dev, i_t, j_t, stride, w_t, m, n, tree, n_tree, lab)
    k = int(n_tree.item())
    return tree[:k], n - k, (lab[:n] if labels else None)


WEIGHTS_TYPES = {"core": 0, "accessory": 1, "euclidean": 2}


def edge_weights_dev(dist_t, edges_t, weights_type="core", n_ref=0, int_offset=0):
    """process_weights (PopPUNK/network.py:646-674) of a model edge list on the device (ppk_edge_weights_dev):
    dist_t the resident float32 [n_rows, 2] matrix, edges_t the int64 [m, 2] list generate_tuples_dev /
    edge_threshold_dev / bgmm_edges_dev made from it (or an (i, j) pair).  n_ref 0: a self (condensed) matrix.
    Returns float32 [m]: core, accessory or the Euclidean norm of every edge's row, bit for bit numpy's."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    if weights_type not in WEIGHTS_TYPES:
        raise ValueError("weights_type must be one of %s" % sorted(WEIGHTS_TYPES))
    i_t, j_t = _edge_cols(edges_t, _EDGES_OR_PAIR, pair=True)
    m, stride = _edge_stream(i_t, j_t, None)
    w = torch.empty(max(m, 1), dtype=torch.float32, device=dist_t.device)
    _dev_call("ppk_edge_weights_dev", dist_t.device, dist_t, dist_t.shape[0], i_t, j_t, stride, m, int(n_ref),
              int(int_offset), WEIGHTS_TYPES[weights_type], w)
    return w[:m]


def dist_pairs(ref, qry=None, kmers=None, random_tbl=None, pairs=None, random_correct=True, jaccard=False,
               counts=False, int_offset=0):
    """Kernel 1 for a LIST of pairs (ppk_dist_pairs_dev): the rows `dist` would write for them, bit
    for bit, without the matrix.  pairs: an int64 [m, 2] CUDA tensor or an (i_t, j_t) pair, edge ids as
    edge_weights_dev reads them (self: two samples of `ref`; otherwise a ref r and n_ref + q; either order, duplicates
    allowed, `int_offset` subtracted).  Returns (out, n_failed): float32 [m, 2], float32 [m, nk] (jaccard) or int32
    [m, nk] (counts), row p for pair p, and a 1-element int64 CUDA tensor counting the listed pairs with fewer than 2
    usable k-mer lengths.  Raises, naming the first offending pair, before anything is written."""
    torch = _torch()
    _check_pair(ref, qry)
    if pairs is None:
        raise ValueError("dist_pairs needs a pair list")
    i_t, j_t = _edge_cols(pairs, _EDGES_OR_PAIR, pair=True)
    m, stride = _edge_stream(i_t, j_t, None)
    if i_t.device.index != ref.device:
        raise ValueError("the pair list is not on the databases' device")
    kmers, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    flags = (FLAG_RANDOM_CORRECT if random_correct else 0) | (FLAG_JACCARD if jaccard else 0) \
        | (FLAG_COUNTS if counts else 0)
    cols = ref.nk if (jaccard or counts) else 2
    dev = "cuda:%d" % ref.device
    out = torch.empty((m, cols), dtype=torch.int32 if counts else torch.float32, device=dev)
    n_failed = torch.zeros(1, dtype=torch.int64, device=dev)
    _dev_call("ppk_dist_pairs_dev", ref.device, ref._h, qry._h if qry is not None else None, kmers, random_tbl, n_clu,
              flags, i_t, j_t, stride, m, int(int_offset), out, n_failed)
    return out, n_failed


def _isqrt(x):
    """floor(sqrt(x)) of a non-negative int64 array, exactly: the double root, then an integer fix-up (above 2^52 the
    double rounds, and a row index of a few million samples is)."""
    x = np.asarray(x, dtype=np.int64)
    r = np.sqrt(x.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        r = np.where(r * r > x, r - 1, r)
    for _ in range(2):
        r = np.where((r + 1) * (r + 1) <= x, r + 1, r)
    return r


def rows_to_pairs(rows, n_ref, n_qry=0):
    """Distance rows -> edge ids, the inverse of the row order (PopPUNK/utils.py:199-226 iterDistRows,
    src/boundary.cpp:22-37) in exact integer arithmetic.  n_qry 0: condensed rows of n_ref samples -> (i, j), i < j;
    otherwise row = q * n_ref + r -> (r, n_ref + q).  numpy int64 [m] in, int64 [m, 2] out."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    n = int(n_ref)
    n_rows = n * int(n_qry) if n_qry else n * (n - 1) // 2
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
        raise ValueError("row index outside [0, %d)" % n_rows)
    out = np.empty((rows.size, 2), dtype=np.int64)
    if n_qry:
        out[:, 0] = rows % n
        out[:, 1] = n + rows // n
        return out
    # rows from the END of the triangle, t = n_rows - 1 - row, lie in reversed row c with c (c + 1) / 2 <= t:
    # c = floor((sqrt(8 t + 1) - 1) / 2), and i = n - 2 - c
    t = (n_rows - 1) - rows
    c = (_isqrt(8 * t + 1) - 1) // 2
    i = n - 2 - c
    out[:, 0] = i
    out[:, 1] = i + 1 + (rows - (i * n - i * (i + 1) // 2))
    return out


def edge_weights_from_sketches(ref, qry, kmers, random_tbl, edges_t, weights_type="core", int_offset=0,
                               random_correct=True):
    """process_weights (PopPUNK/network.py:646-674; scripts/poppunk_add_weights.py) of an edge list with no matrix:
    the edges' distances come from the resident sketches (dist_pairs).  Returns float32 [m], bit for bit
    edge_weights_dev(dist(...), edges_t, ...)."""
    torch = _torch()
    if weights_type not in WEIGHTS_TYPES:
        raise ValueError("weights_type must be one of %s" % sorted(WEIGHTS_TYPES))
    d, _ = dist_pairs(ref, qry, kmers, random_tbl, edges_t, random_correct=random_correct, int_offset=int_offset)
    return edge_weights_of_rows(d, weights_type)


def edge_weights_of_rows(rows_t, weights_type="core"):
    """process_weights of edges whose (core, accessory) rows are at hand -- the rows of dist_edges_rows, or of
    dist_pairs: float32 [m], the column for "core" / "accessory", the row norms for "euclidean".  What
    edge_weights_from_sketches returns for those edges, bit for bit, with no further pass over the sketches."""
    torch = _torch()
    if weights_type not in WEIGHTS_TYPES:
        raise ValueError("weights_type must be one of %s" % sorted(WEIGHTS_TYPES))
    _check_tensor(rows_t, "rows must be a contiguous float32 [m, 2] CUDA tensor", torch.float32, shape=(None, 2))
    d = rows_t
    if weights_type != "euclidean":
        return d[:, WEIGHTS_TYPES[weights_type]].contiguous()
    w = torch.empty(max(d.shape[0], 1), dtype=torch.float32, device=d.device)
    _dev_call("ppk_row_norms_dev", d.device, d, d.shape[0], w)
    return w[:d.shape[0]]


def sweep_boundaries_1d(offsets, slope, x0, y0, x1, y1):
    """The boundaries of a 1-D sweep (ppk_sweep_boundaries_1d; no device): (x_max, y_max) float32 [n_off] of the sorted
    offsets along (x0, y0) -> (x1, y1), the values thresholdIterate1D computes (src/boundary.cpp:161-186)."""
    off = np.ascontiguousarray(offsets, dtype=np.float64)
    x_max = np.empty(off.size, dtype=np.float32)
    y_max = np.empty(off.size, dtype=np.float32)
    _lib.call("ppk_sweep_boundaries_1d", off.ctypes.data_as(C.POINTER(C.c_double)), off.size, int(slope), float(x0),
              float(y0), float(x1), float(y1), x_max.ctypes.data_as(C.POINTER(C.c_float)),
              y_max.ctypes.data_as(C.POINTER(C.c_float)))
    return x_max, y_max


def sweep_levels_dev(rows_t, x_max, y_max, slope, out=None):
    """The sweep level of listed rows (ppk_sweep_levels_dev): int32 [m], for row p of the float32 [m, 2] CUDA tensor
    the first of the boundaries (x_max[o], y_max[o]) (host arrays) that holds it -- the offset index
    threshold_iterate_1d_dev / _2d_dev give a row with those coordinates -- and len(x_max) where none does."""
    torch = _torch()
    if not (rows_t.is_cuda and rows_t.dtype == torch.float32 and rows_t.dim() == 2 and rows_t.shape[1] == 2
            and rows_t.is_contiguous()):
        raise TypeError("rows must be a contiguous float32 [m, 2] CUDA tensor")
    x_max = np.ascontiguousarray(x_max, dtype=np.float32)
    y_max = np.ascontiguousarray(y_max, dtype=np.float32)
    if x_max.ndim != 1 or x_max.shape != y_max.shape:
        raise ValueError("x_max and y_max must be 1-D arrays of one length")
    m = int(rows_t.shape[0])
    if out is None:
        out = torch.empty(m, dtype=torch.int32, device=rows_t.device)
    _dev_call("ppk_sweep_levels_dev", rows_t.device, rows_t, m, x_max.ctypes.data_as(C.POINTER(C.c_float)),
              y_max.ctypes.data_as(C.POINTER(C.c_float)), x_max.size, int(slope), out)
    return out


NJ_SQUARE, NJ_LONG = 0, 1


def nj_dev(src, n=None, col=0):
    """Neighbour joining of a core-distance matrix on the device (ppk_nj_dev), read in place: a
    float32 [n, n] CUDA square, or the resident long form, [n_pairs] or column col of [n_pairs, k].  Only the strictly
    lower triangle is read.  Returns (join int64 [n-1, 2], len float64 [n-1, 2]) CUDA tensors: row t < n-2 is join
    t's node ids (a, b) -- samples 0 .. n-1, node n + t' made by join t' -- and (len_a, len_b); row n-2 is the final
    edge (the two nodes left, its length twice).  n = 1 gives empty tensors."""
    torch = _torch()
    _check_tensor(src, "the matrix must be a contiguous float32 CUDA tensor: [n, n] square or [n_pairs(, k)] long",
                  torch.float32, dim=(1, 2))
    if src.dim() == 2 and src.shape[0] == src.shape[1]:
        kind, stride, col, nn = NJ_SQUARE, 1, 0, int(src.shape[0])
    else:
        kind, stride, col, nn = NJ_LONG, (1 if src.dim() == 1 else int(src.shape[1])), int(col), \
            _samples_of(int(src.shape[0]))
        if nn * (nn - 1) // 2 != int(src.shape[0]):
            raise ValueError("a long-form matrix must have n(n-1)/2 rows")
        if not 0 <= col < stride:
            raise ValueError("col must index a column of the long form")
    if n is not None and int(n) != nn:
        raise ValueError("n = %d does not match the matrix (%d samples)" % (int(n), nn))
    join = torch.empty((max(nn - 1, 0), 2), dtype=torch.int64, device=src.device)
    ln = torch.empty((max(nn - 1, 0), 2), dtype=torch.float64, device=src.device)
    _dev_call("ppk_nj_dev", src.device, src, kind, stride, col, nn, join, ln)
    return join, ln


def nj(square, device_id=0):
    """ppk_nj: neighbour joining of a host float32 [n, n] matrix (lower triangle read).  Returns numpy
    (join int64 [n-1, 2], len float64 [n-1, 2]) as nj_dev."""
    sq = np.ascontiguousarray(square, dtype=np.float32)
    if sq.ndim != 2 or sq.shape[0] != sq.shape[1]:
        raise ValueError("the matrix must be square")
    nn = int(sq.shape[0])
    join = np.empty((max(nn - 1, 0), 2), dtype=np.int64)
    ln = np.empty((max(nn - 1, 0), 2), dtype=np.float64)
    _lib.call("ppk_nj", sq, nn, int(device_id), join, ln)
    return join, ln


EMBED_WORKERS = 65536     # workers per iteration as mandrake's GPU call sets them (PopPUNK/mandrake.py:77)


def _embed_lists(i_t, j_t, n, what):
    torch = _torch()
    n = int(n)
    for t in (i_t, j_t):
        _check_tensor(t, "%s: i and j must be contiguous int64 CUDA vectors" % what, torch.int64, dim=1)
    m = int(i_t.numel())
    if int(j_t.numel()) != m or n < 2 or m % n or not 1 <= m // n <= n - 1:
        raise ValueError("%s: lists of n*k entries with n >= 2 and 1 <= k <= n - 1 expected (n = %d, %d entries)"
                         % (what, n, m))
    return m // n


def embed_weights_dev(i_t, j_t, dist_t, n, perplexity=20.0, weights=False):
    """The embedding's calibration on the device (ppk_embed_weights_dev) from neighbour lists in
    get_kNN_distances form (CUDA i, j int64 and dist float32 [n*k], row i = e // k).  Returns P, float64 [n*k] with
    sum 1, and with weights=True also the integer sampling weights rint(P * 2^52) as int64 (uint64 bits)."""
    torch = _torch()
    k = _embed_lists(i_t, j_t, n, "embed_weights_dev")
    _check_tensor(dist_t, "embed_weights_dev: dist must be a contiguous float32 CUDA vector as long as i",
                  torch.float32, numel=int(i_t.numel()))
    dev = i_t.device
    P = torch.empty(int(i_t.numel()), dtype=torch.float64, device=dev)
    c = torch.empty(int(i_t.numel()), dtype=torch.int64, device=dev) if weights else None
    _dev_call("ppk_embed_weights_dev", dev, i_t, j_t, dist_t, int(n), k, float(perplexity), P, c)
    return (P, c) if weights else P


def embed_dev(i_t, j_t, P_t, n, seed, max_iter=10000000, n_repu=5, eta0=1.0, workers=EMBED_WORKERS):
    """The embedding's loop on the device (ppk_embed_dev): lists and P (embed_weights_dev) -> Y,
    a float64 [n, 2] CUDA tensor.  min(workers, n) workers per iteration, round(max_iter / that) iterations."""
    torch = _torch()
    k = _embed_lists(i_t, j_t, n, "embed_dev")
    _check_tensor(P_t, "embed_dev: P must be a contiguous float64 CUDA vector as long as i", torch.float64,
                  numel=int(i_t.numel()))
    Y = torch.empty((int(n), 2), dtype=torch.float64, device=i_t.device)
    _dev_call("ppk_embed_dev", i_t.device, i_t, j_t, P_t, int(n), k, int(seed) & ((1 << 64) - 1), int(max_iter),
              int(n_repu), float(eta0), int(workers), Y)
    return Y


def embed(i, j, dist, n, seed, perplexity=20.0, max_iter=10000000, n_repu=5, eta0=1.0, workers=EMBED_WORKERS,
          device_id=0):
    """ppk_embed: embed_weights_dev then embed_dev on host arrays (numpy or sequences, get_kNN_distances form).
    Returns numpy (P float64 [n*k], Y float64 [n, 2])."""
    ii = np.ascontiguousarray(i, dtype=np.int64).ravel()
    jj = np.ascontiguousarray(j, dtype=np.int64).ravel()
    dd = np.ascontiguousarray(dist, dtype=np.float32).ravel()
    n, m = int(n), int(ii.size)
    if jj.size != m or dd.size != m or n < 2 or m % n or not 1 <= m // n <= n - 1:
        raise ValueError("embed: lists of n*k entries with n >= 2 and 1 <= k <= n - 1 expected (n = %d, %d entries)"
                         % (n, m))
    P = np.empty(m, dtype=np.float64)
    Y = np.empty((n, 2), dtype=np.float64)
    _lib.call("ppk_embed", ii, jj, dd, n, m // n, float(perplexity), int(seed) & ((1 << 64) - 1), int(max_iter),
              int(n_repu), float(eta0), int(workers), int(device_id), P, Y)
    return P, Y


def _samples_of(n_rows):
    n = int((1 + (1 + 8 * n_rows) ** 0.5) // 2)
    while n * (n - 1) // 2 > n_rows:
        n -= 1
    while (n + 1) * n // 2 <= n_rows:
        n += 1
    if n * (n - 1) // 2 != n_rows:
        raise ValueError("row count is not n(n-1)/2 for any n (self/condensed matrix expected)")
    return n


def _sweep_scores(dist_t, sweep, n_off, score_idx=0, betweenness_sample=None, seed=0):
    return _sweep_scores_of(_samples_of(dist_t.shape[0]), sweep, n_off, score_idx, betweenness_sample, seed)


def _sweep_scores_of(n, sweep, n_off, score_idx=0, betweenness_sample=None, seed=0):
    """(stats, growNetwork's list) of a sweep's (i, j, offset index) over n samples, the edges in any order."""
    from . import refine
    i, j, o = sweep
    if score_idx == 0:
        stats, _ = network_sweep_dev(i, j, o, n, n_off)
        st = stats.cpu().numpy()
        return stats, refine.grow_scores(st, n)
    if betweenness_sample is None:
        stats, bt, _, _ = network_summary_dev(i, j, o, n, n_off)
    else:
        stats, bt, _, _ = network_summary_sampled_dev(i, j, o, n, n_off, sources=betweenness_sample, seed=seed)
    return stats, refine.grow_scores(stats.cpu().numpy(), n, score_idx, bt=bt.cpu().numpy())


def _check_score_idx(score_idx):
    if score_idx not in (0, 1, 2):
        raise ValueError("score_idx must be 0, 1 or 2")
    return int(score_idx)


def refine_sweep_scores_dev(dist_t, offsets, slope, x0, y0, x1, y1, score_idx=0, betweenness_sample=None, seed=0):
    """thresholdIterate1D + growNetwork on a resident float32 [n,2] CUDA matrix, without the edge list leaving the
    device (PopPUNK/refine.py:190-202).  Returns (stats int64 [len(offsets), 4] CUDA, growNetwork's score list).
    score_idx 1 / 2 (refine's --score-idx) scores with the mean / size-weighted mean betweenness (network_summary_dev;
    with betweenness_sample = k, network_summary_sampled_dev from at most k sources per component under `seed`);
    0 leaves betweenness out, as growNetwork does."""
    score_idx = _check_score_idx(score_idx)
    off = np.ascontiguousarray(offsets, dtype=np.float64).ravel()
    return _sweep_scores(dist_t, threshold_iterate_1d_dev(dist_t, off, slope, x0, y0, x1, y1), off.size, score_idx,
                         betweenness_sample, seed)


def refine_sweep_scores_2d_dev(dist_t, x_max, y_max, score_idx=0, betweenness_sample=None, seed=0):
    """thresholdIterate2D + growNetwork for one y (PopPUNK/refine.py:587-595), as refine_sweep_scores_dev."""
    score_idx = _check_score_idx(score_idx)
    xm = np.ascontiguousarray(x_max, dtype=np.float32).ravel()
    return _sweep_scores(dist_t, threshold_iterate_2d_dev(dist_t, xm, y_max), xm.size, score_idx, betweenness_sample,
                         seed)


def refine_score_dev(dist_t, slope, x_max, y_max):
    """The counts of ONE refine boundary on a resident float32 [n(n-1)/2, 2] CUDA matrix (ppk_refine_score_dev,
    DESIGN.md 3.14): int64 numpy [4] = edges, components, triangles, connected triples of the graph of every row with
    line_dist <= 0 -- edge_threshold_dev + network_stats_dev in one call, without the edge list."""
    torch = _torch()
    _check_dist_tensor(dist_t)
    stats = torch.empty(4, dtype=torch.int64, device=dist_t.device)
    _dev_call("ppk_refine_score_dev", dist_t.device, dist_t, dist_t.shape[0], int(slope), float(x_max), float(y_max),
              stats)
    return stats.cpu().numpy()


def refine_score(X, slope, x_max, y_max, device_id=0):
    """refine_score_dev on a host float32 [n(n-1)/2, 2] array (ppk_refine_score)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] != 2:
        raise ValueError("distances must be a float32 [n, 2] array")
    stats = np.zeros(4, dtype=np.int64)
    _lib.call("ppk_refine_score", X, X.shape[0], int(slope), float(x_max), float(y_max), int(device_id), stats)
    return stats


class RefineLocal:
    """The bracket handle of refine's local search (ppk_refine_local_*): the rows of a resident
    condensed matrix sorted once into base / candidates / never against two nested lines; `eval(x_max, y_max)` then
    gives refine_score_dev's counts for any line between them.  `create` returns None when the two lines are not
    nested (the caller scores with refine_score_dev).  `split` = (base, candidates, never) rows."""

    def __init__(self, handle, device):
        self._h, self.device = handle, device
        split = (C.c_ulonglong * 3)()
        _lib.call("ppk_refine_local_stats", self._h, split)
        self.split = tuple(int(v) for v in split)

    @classmethod
    def create(cls, dist_t, slope, x_lo, y_lo, x_hi, y_hi):
        _check_dist_tensor(dist_t)
        h = C.c_void_p()
        rc = _dev_call("ppk_refine_local_create_dev", dist_t.device, dist_t, dist_t.shape[0], int(slope), float(x_lo),
                       float(y_lo), float(x_hi), float(y_hi), then=(C.byref(h),), accept=(_lib.REFINE_NOT_NESTED,))
        return None if rc == _lib.REFINE_NOT_NESTED else cls(h, dist_t.device)

    def eval(self, x_max, y_max):
        torch = _torch()
        if self._h is None:
            raise RuntimeError("the bracket handle is closed")
        stats = torch.empty(4, dtype=torch.int64, device=self.device)
        _dev_call("ppk_refine_local_eval_dev", self.device, self._h, float(x_max), float(y_max), stats)
        return stats.cpu().numpy()

    def close(self):
        if self._h is not None:
            _lib.lib().ppk_refine_local_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def long_to_square_dev(dist_t, col, n):
    """pp_sketchlib.longToSquare of one column of the resident [n_pairs,2] matrix -> [n,n] CUDA."""
    torch = _torch()
    out = torch.empty((n, n), dtype=torch.float32, device=dist_t.device)
    _dev_call("ppk_long_to_square_dev", dist_t.device, dist_t, dist_t.shape[1], int(col), n, out)
    return out


def prune_long_dev(dist_t, n, keep):
    """Long-form matrix of the kept samples out of the resident long-form matrix of n samples
    (the row copy of PopPUNK/qc.py:58-83 as one gather).  keep: ascending sample indices."""
    torch = _torch()
    keep_t = torch.as_tensor(np.ascontiguousarray(keep, dtype=np.int64), device=dist_t.device)
    m = int(keep_t.shape[0])
    if m and (int(keep_t.min()) < 0 or int(keep_t.max()) >= n or
              (m > 1 and bool((keep_t[1:] <= keep_t[:-1]).any()))):
        raise RuntimeError("kept indices must be strictly ascending and inside the matrix")
    cols = 1 if dist_t.dim() == 1 else int(dist_t.shape[1])
    shape = (m * (m - 1) // 2,) if dist_t.dim() == 1 else (m * (m - 1) // 2, cols)
    out = torch.empty(shape, dtype=torch.float32, device=dist_t.device)
    _dev_call("ppk_prune_long_dev", dist_t.device, dist_t, n, cols, keep_t, m, out)
    return out


def prune_query_rows_dev(qr_t, n_ref, keep_q):
    """Row blocks (row = q*n_ref + r) of the kept queries (PopPUNK/qc.py:121-135)."""
    torch = _torch()
    keep_t = torch.as_tensor(np.ascontiguousarray(keep_q, dtype=np.int64), device=qr_t.device)
    m = int(keep_t.shape[0])
    cols = 1 if qr_t.dim() == 1 else int(qr_t.shape[1])
    n_qry = qr_t.shape[0] // max(n_ref, 1)
    if m and (int(keep_t.min()) < 0 or int(keep_t.max()) >= n_qry):
        raise RuntimeError("kept query index outside the matrix")
    shape = (m * n_ref,) if qr_t.dim() == 1 else (m * n_ref, cols)
    out = torch.empty(shape, dtype=torch.float32, device=qr_t.device)
    for lo in range(0, m, 65535):
        hi = min(m, lo + 65535)
        _dev_call("ppk_prune_query_rows_dev", qr_t.device, qr_t, n_ref, cols, keep_t[lo:], hi - lo,
                  out[lo * n_ref:])
    return out


def knn_ref_query(ref, qry, kmers, random_tbl, knn, dist_col=0, random_correct=True, info=None):
    """ppk_knn_sketches_rq_dev: for every reference its knn nearest queries (numbered n_ref + q) and for every
    query its knn nearest references, one pass over the rectangle's tiles.  CUDA tensors (i, j, dist) of length
    (n_ref + n_qry) * knn, references first."""
    _check_pair(ref, qry)
    oi, oj, od = _neighbour_outputs((ref.n + qry.n) * knn, "cuda:%d" % ref.device)
    kmers_a, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    n_cand = C.c_ulonglong(0)
    _dev_call("ppk_knn_sketches_rq_dev", ref.device, ref._h, qry._h, kmers_a, random_tbl, n_clu,
              FLAG_RANDOM_CORRECT if random_correct else 0, int(knn), int(dist_col), oi, oj, od, C.byref(n_cand))
    if info is not None:
        info["candidates"] = int(n_cand.value)
    return oi, oj, od


def knn_from_sketches(db, kmers, random_tbl, knn, dist_col=0, random_correct=True,
                      band_items=1 << 31, method="auto", info=None):
    """k nearest neighbours of every sample straight from the resident sketches (what
    get_kNN_distances(longToSquare(queryDatabase(...)[:, dist_col])) gives, PopPUNK/models.py:
    1215-1222), entirely on the device.  Returns CUDA tensors (i, j, dist) of length n*knn.

    method "tiles" (the default where it applies: bbits 14, knn <= 32, up to 128 k-mer lengths):
        kernel 1's tiles emit neighbour candidates under per-sample bounds and a sort + selection
        pass finishes (ppk_knn_sketches_dev): the upper triangle is compared once and no distance
        matrix -- long or square -- is ever built.  `info` (a dict) receives the candidate count.
    method "square": upper triangle -> n x n square -> per-row selection (8 n^2 bytes of HBM).
    method "bands":  bands of query rows against all refs (row = q*n + r; both triangles: twice the
        compare work, one band of the matrix at a time).
    "auto" falls back to "square" while n*n <= band_items, else "bands", where "tiles" does not apply."""
    torch = _torch()
    n = db.n
    dev = "cuda:%d" % db.device
    oi, oj, od = _neighbour_outputs(n * knn, dev)
    if method == "auto":
        # (any k list the tile kernel takes: lists of more than 128 count bits run its windowed instantiation)
        tiles_ok = db.bbits == 14 and 1 <= knn <= 32 and db.nk <= 128 and n > 1
        method = "tiles" if tiles_ok else ("square" if n * n <= band_items else "bands")
    if method == "tiles":
        kmers_a, random_tbl, n_clu = _prep_tables(kmers, random_tbl, db.nk)
        n_cand = C.c_ulonglong(0)
        _dev_call("ppk_knn_sketches_dev", db.device, db._h, kmers_a, random_tbl, n_clu,
                  FLAG_RANDOM_CORRECT if random_correct else 0, int(knn), int(dist_col), oi, oj, od, C.byref(n_cand))
        if info is not None:
            info["candidates"] = int(n_cand.value)
        return oi, oj, od
    if method == "square" and n > 1:
        tri, _ = dist(db, None, kmers, random_tbl, random_correct=random_correct)
        sq = long_to_square_dev(tri, dist_col, n)
        del tri
        _dev_call("ppk_knn_dev", db.device, sq, n, int(knn), oi, oj, od)
        return oi, oj, od
    band = max(64, min(n, (band_items // max(n, 1)) // 64 * 64))
    buf = torch.empty((min(band, n) * n, 2), dtype=torch.float32, device=dev)
    for qb in range(0, n, band):
        qe = min(n, qb + band)
        block = buf[:(qe - qb) * n]
        dist(db, db, kmers, random_tbl, random_correct=random_correct, q_begin=qb, q_end=qe,
             out=block)
        _dev_call("ppk_knn_rect_dev", db.device, block, 2, int(dist_col), qe - qb, n, qb, int(knn), oi[qb * knn:],
                  oj[qb * knn:], od[qb * knn:])
    return oi, oj, od


def extend_from_sketches(rr_mat, ref, qry, kmers, random_tbl, knn, dist_col=0, random_correct=True):
    """poppunk_refine.extend(rr_mat, qq_mat, qr_mat, kNN) with the resident sketches of the references and
    the queries in the place of the two dense matrices (ppk_extend_sketches): -> (i, j, dist) numpy arrays,
    queries numbered n_ref + q."""
    import numpy as np
    refs = [ref] if isinstance(ref, SketchDB) else list(ref)        # one pair of databases per device
    qrys = [qry] if isinstance(qry, SketchDB) else list(qry)
    if len(refs) != len(qrys):
        raise ValueError("one query database per reference database")
    for a, b in zip(refs, qrys):
        _check_pair(a, b)
    ref, qry = refs[0], qrys[0]
    r, c, d = rr_mat
    r = np.ascontiguousarray(np.asarray(r).astype(np.int64, copy=False)).ravel()
    c = np.ascontiguousarray(np.asarray(c).astype(np.int64, copy=False)).ravel()
    d = np.ascontiguousarray(np.asarray(d).astype(np.float32, copy=False)).ravel()
    kmers, random_tbl, n_clu = _prep_tables(kmers, random_tbl, ref.nk)
    cap = max(int(knn) * (ref.n + qry.n), 1)
    oi, oj, od = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.float32)
    n = C.c_size_t(0)
    rh = (C.c_void_p * len(refs))(*[x._h.value for x in refs])
    qh = (C.c_void_p * len(refs))(*[x._h.value for x in qrys])
    _lib.call("ppk_extend_sketches_dbs", r, c, d, r.size, rh, qh, len(refs), kmers, random_tbl, n_clu,
              FLAG_RANDOM_CORRECT if random_correct else 0, int(knn), int(dist_col), oi, oj, od, cap, C.byref(n),
              what="ppk_extend_sketches")
    return oi[:n.value], oj[:n.value], od[:n.value]


def knn_candidates(db, kmers, random_tbl, knn, dist_col=0, random_correct=True, q_begin=0, q_end=None,
                   cap=None):
    """Neighbour candidates of one band of query rows (ppk_knn_candidates_dev): CUDA tensors
    (keys int32 [m] = sample, vals int64 [m] = distance bits << 32 | other sample)."""
    torch = _torch()
    q_end = db.n if q_end is None else int(q_end)
    kmers_a, random_tbl, n_clu = _prep_tables(kmers, random_tbl, db.nk)
    dev = "cuda:%d" % db.device
    rows = rows_in_band(db.n, 0, q_begin, q_end)
    if cap is None:
        cap = min(2 * rows, max(1 << 20, (256 + 256 * knn) * max(q_end - q_begin, 1) * 2))
    while True:
        keys = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        vals = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        n_cand = C.c_ulonglong(0)
        rc = _dev_call("ppk_knn_candidates_dev", db.device, db._h, kmers_a, random_tbl, n_clu,
                       FLAG_RANDOM_CORRECT if random_correct else 0, int(knn), int(dist_col), int(q_begin), q_end,
                       keys, vals, cap, C.byref(n_cand), accept=(_lib.ERR_CAPACITY,))
        m = int(n_cand.value)
        if rc == _lib.OK:
            return keys[:m], vals[:m]
        cap = m + m // 4 + 1024


def knn_select(keys, vals, n, knn):
    """Every sample's knn smallest (distance, column) keys out of a candidate list
    (ppk_knn_select_dev) -> (i, j, dist) CUDA tensors of length n*knn."""
    oi, oj, od = _neighbour_outputs(n * knn, keys.device)
    _dev_call("ppk_knn_select_dev", keys.device, keys.contiguous(), vals.contiguous(), int(keys.shape[0]), int(n),
              int(knn), oi, oj, od)
    return oi, oj, od


def knn_band(db, kmers, random_tbl, knn, dist_col=0, random_correct=True, q_begin=0, q_end=None, info=None):
    """ppk_knn_sketches_band_dev: the best knn per sample among the pairs of one band of the triangle's rows;
    CUDA tensors (j int64, dist float32) of length n * knn, unfilled slots j = -1."""
    q_end = db.n if q_end is None else int(q_end)
    oi, oj, od = _neighbour_outputs(db.n * knn, "cuda:%d" % db.device)
    kmers_a, random_tbl, n_clu = _prep_tables(kmers, random_tbl, db.nk)
    n_cand = C.c_ulonglong(0)
    _dev_call("ppk_knn_sketches_band_dev", db.device, db._h, kmers_a, random_tbl, n_clu,
              FLAG_RANDOM_CORRECT if random_correct else 0, int(knn), int(dist_col), int(q_begin), q_end, oi, oj, od,
              C.byref(n_cand))
    if info is not None:
        info["candidates"] = int(n_cand.value)
    return oj, od


_KNN_NONE = (1 << 63) - 1      # key of an unfilled slot: sorts behind every (distance bits << 32 | j)


def knn_merge_lists(keys, n, knn):
    """Per-band neighbour lists as int64 keys [bands, n * knn] (distance bits << 32 | j, unfilled = 2^63 - 1)
    -> (i, j, dist) of the whole job: per sample the knn smallest keys of all bands, i.e. the reference's stable
    order by distance, ties to the lower index (src/extend.cpp:266-279); slots no band could fill keep the
    reference's filler (i, 0, 0.0)."""
    torch = _torch()
    bands = keys.shape[0]
    per = keys.view(bands, n, knn).permute(1, 0, 2).reshape(n, bands * knn)
    best = torch.sort(per, dim=1).values[:, :knn].reshape(-1)
    none = best == _KNN_NONE
    oj = torch.where(none, torch.zeros_like(best), best & 0xFFFFFFFF)
    od = torch.where(none, torch.zeros_like(best), best >> 32).to(torch.int32).view(torch.float32)
    oi = torch.arange(n, device=keys.device, dtype=torch.int64).repeat_interleave(knn)
    return oi, oj, od


def knn_sharded(db, kmers, random_tbl, knn, rank, world_size, dist_col=0, random_correct=True, group=None,
                band_fn=None):
    """k nearest neighbours of every sample on N GPUs: every rank holds the full resident sketches, takes a
    band of the triangle (the band split of the distance job: equal pair counts) and reduces it to the best
    knn per sample ON ITS DEVICE (`knn_band`: the staged candidate flow of the single-GPU call); what travels to
    rank 0 is one int64 key per slot -- n * knn * 8 bytes per rank, whatever the candidate stream was -- and
    rank 0 merges (`knn_merge_lists`).  Returns (i, j, dist) on rank 0, None elsewhere.
    `band_fn(q_begin, q_end) -> (j, dist)` overrides the HIP launch (CPU gloo tests of the exchange)."""
    torch = _torch()
    import torch.distributed as dist_
    bounds = shard_bounds(db.n, 0, world_size)
    qb, qe = bounds[rank], bounds[rank + 1]
    oj, od = band_fn(qb, qe) if band_fn is not None else knn_band(db, kmers, random_tbl, knn, dist_col, random_correct, qb, qe)
    keys = (od.contiguous().view(torch.int32).to(torch.int64) << 32) | oj
    keys = torch.where(oj < 0, torch.full_like(keys, _KNN_NONE), keys)
    if world_size > 1:
        nccl = str(dist_.get_backend(group)).lower() == "nccl"
        send = keys if nccl else keys.cpu()
        dst = 0 if group is None else dist_.get_global_rank(group, 0)
        got = [torch.empty_like(send) for _ in range(world_size)] if rank == 0 else None
        dist_.gather(send, got, dst=dst, group=group)
        if rank != 0:
            return None
        keys = torch.stack(got).to(keys.device)
    else:
        keys = keys.unsqueeze(0)
    return knn_merge_lists(keys, db.n, knn)


# ---- multi-GPU: one process per GPU, band-sharded pair space, gather to rank 0 -------------

def shard_bounds(n_ref, n_qry, world_size):
    return band_split(n_ref, n_qry, world_size)


def gather_bands(local, rows_per_rank, cols, dtype, device, rank, world_size, dst=0, group=None):
    """Gather variable-height row blocks to `dst` with grouped point-to-point
    send/recv (RCCL over xGMI on GPUs: each peer streams over its own link into the
    final matrix, so rank `dst` receives every band directly at its row offset and
    no staging copy or re-ordering pass is needed).  Returns the full tensor on
    `dst`, None elsewhere."""
    torch = _torch()
    import torch.distributed as dist_
    if world_size == 1:
        return local
    if local.is_cuda and str(dist_.get_backend(group)).lower() != "nccl":
        torch.cuda.current_stream(local.device).synchronize()      # gloo: no stream ordering (see ShardedQuery.run)
    if rank == dst:
        total = int(sum(rows_per_rank))
        full = torch.empty((total, cols), dtype=dtype, device=device)
        offs = np.concatenate([[0], np.cumsum(rows_per_rank)]).astype(np.int64)
        full[offs[dst]:offs[dst + 1]].copy_(local)
        ops = []
        for src in range(world_size):
            if src == dst or rows_per_rank[src] == 0:
                continue
            ops.append(dist_.P2POp(dist_.irecv, full[offs[src]:offs[src + 1]], src, group))
        if ops:
            for req in dist_.batch_isend_irecv(ops):
                req.wait()
        return full
    if rows_per_rank[rank] > 0:
        for req in dist_.batch_isend_irecv([dist_.P2POp(dist_.isend, local.contiguous(), dst, group)]):
            req.wait()
    return None


def sub_bands(q_begin, q_end, n_chunks):
    """Cut a band of query rows into n_chunks contiguous sub-bands (edges on 64-query tiles)."""
    edges = [q_begin]
    for c in range(1, n_chunks):
        e = q_begin + (q_end - q_begin) * c // n_chunks
        e = min(q_end, (e + 32) // 64 * 64)
        edges.append(max(e, edges[-1]))
    edges.append(q_end)
    return edges


class ShardedQuery:
    """The N-GPU distance job of BASELINE configs 3/4: one process per GPU, every rank holds
    the full resident sketches, the pair space is band-split over ranks, and the distance
    blocks are gathered into the PopPUNK-ordered matrix on rank 0.

    The gather is pipelined under the compute: each rank's band is cut into `n_chunks`
    sub-bands; as soon as sub-band c has been enqueued its block is handed to an asynchronous
    send (RCCL runs it on its own stream after the producing kernel), while the next
    sub-band computes.  Rank 0 posts, per chunk, ONE grouped receive from all peers, each
    landing directly at its row offset of the final matrix (a band is a contiguous row
    range, so there is no staging copy or reorder).  On xGMI every peer has its own link to
    the root, so the seven inbound streams run in parallel.

    `band_fn(q_begin, q_end, out)` overrides the HIP launch (CPU gloo tests)."""

    def __init__(self, ref, qry, rank, world_size, n_chunks=4, cols=2, dtype=None, device=None,
                 group=None, weights=None):
        torch = _torch()
        self.ref, self.qry = ref, qry
        self.rank, self.world = rank, world_size
        self.group = group
        self.n_qry = qry.n if qry is not None else 0
        self.n_chunks = n_chunks
        self.cols = cols
        self.dtype = dtype or torch.float32
        self.device = device if device is not None else "cuda:%d" % ref.device
        self.out = None
        self.n_failed = None
        self.weights = [1.0] * world_size if weights is None else [float(x) for x in weights]
        self._layout(shard_bounds(ref.n, self.n_qry, world_size) if weights is None
                     else band_split_weighted(ref.n, self.n_qry, self.weights))

    def _layout(self, bounds):
        """Bands -> sub-bands -> row counts and offsets; (re)allocates the local result."""
        torch = _torch()
        self.bounds = [int(b) for b in bounds]
        self.chunks = [sub_bands(self.bounds[r], self.bounds[r + 1], self.n_chunks)
                       for r in range(self.world)]
        self.rows = [[rows_in_band(self.ref.n, self.n_qry, ch[c], ch[c + 1]) for c in range(self.n_chunks)]
                     for ch in self.chunks]
        self.band_rows = [sum(r) for r in self.rows]
        self.total_rows = sum(self.band_rows)
        # rank 0 owns the full matrix and computes its own band in place; peers own a band
        n_local = self.total_rows if self.rank == 0 else self.band_rows[self.rank]
        if self.out is None or self.out.shape[0] != n_local:
            self.out = None          # release before allocating the new one
            self.out = torch.empty((n_local, self.cols), dtype=self.dtype, device=self.device)
        self.band_off = [0]
        for r in range(self.world):
            self.band_off.append(self.band_off[-1] + self.band_rows[r])

    def _nccl(self):
        import torch.distributed as dist_
        return str(dist_.get_backend(self.group)).lower() == "nccl"

    def _chunk_view(self, r, c):
        """Rows of chunk c of rank r's band inside self.out (rank 0: global offsets)."""
        start = sum(self.rows[r][:c]) + (self.band_off[r] if self.rank == 0 else 0)
        return self.out[start:start + self.rows[r][c]]

    def run(self, kmers=None, random_tbl=None, random_correct=True, band_fn=None):
        """One whole-job step.  Returns the full matrix on rank 0 (None elsewhere)."""
        import time
        import torch.distributed as dist_
        torch = _torch()
        pending = []
        timing = getattr(self, "_time_compute", False)
        on_gpu = str(self.device).startswith("cuda")
        if timing:
            self._compute_s = 0.0
            if on_gpu:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(torch.cuda.current_stream(self.device))
        for c in range(self.n_chunks):
            qb, qe = self.chunks[self.rank][c], self.chunks[self.rank][c + 1]
            view = self._chunk_view(self.rank, c)
            if view.shape[0]:
                t_c = time.perf_counter()
                if band_fn is not None:
                    band_fn(qb, qe, view)
                else:
                    if self.n_failed is None:      # failed fits of every step so far, this rank's bands
                        self.n_failed = torch.zeros(1, dtype=torch.int64, device=self.device)
                    dist(self.ref, self.qry, kmers, random_tbl, random_correct=random_correct,
                         q_begin=qb, q_end=qe, out=view, n_failed=self.n_failed)
                if timing and not on_gpu:
                    self._compute_s += time.perf_counter() - t_c
            if self.world == 1:
                continue
            if on_gpu and not self._nccl():
                # gloo (debugging transport) reads a CUDA tensor's memory from the host with no
                # stream ordering; RCCL orders the send after the producing kernel by itself
                torch.cuda.current_stream(self.device).synchronize()
            if self.rank == 0:
                ops = [dist_.P2POp(dist_.irecv, self._chunk_view(s, c), s, self.group)
                       for s in range(1, self.world) if self.rows[s][c] > 0]
            else:
                ops = [dist_.P2POp(dist_.isend, view, 0, self.group)] if view.shape[0] else []
            if ops:
                pending.extend(dist_.batch_isend_irecv(ops))
        if timing and on_gpu:
            ev1.record(torch.cuda.current_stream(self.device))
        for req in pending:
            req.wait()
        if timing and on_gpu:
            ev1.synchronize()
            self._compute_s = ev0.elapsed_time(ev1) * 1e-3
        return self.out if self.rank == 0 else None

    def rebalance(self, kmers=None, random_tbl=None, random_correct=True, band_fn=None, steps=2):
        """Re-cut the bands so that every rank's part of a step takes equally long.

        With equal bands a step lasts as long as the slowest peer-to-root transfer: a peer
        produces 8 B per pair faster than its one link to the root carries them, while the root's
        own band needs no transfer at all.  One measured step gives each rank's rate -- the root:
        pairs per second of compute; a peer: pairs per second until its last block has been
        handed over -- and the new shares are proportional to the rates (the model is linear,
        so one or two calls converge; where the links keep up with the kernels the rates are
        equal and so stay the bands).  Collective: every rank must call it the same number of
        times.  Returns the new shares (fractions of the pair space per rank)."""
        import time
        import torch.distributed as dist_
        torch = _torch()
        if self.world == 1:
            return [1.0]
        on_gpu = str(self.device).startswith("cuda")

        def sync():
            if on_gpu:
                torch.cuda.synchronize(self.device)

        mine = 0.0
        self._time_compute = True
        try:
            for _ in range(max(1, steps)):           # the last step's time is the one used
                dist_.barrier(self.group)
                sync()
                t0 = time.perf_counter()
                self.run(kmers, random_tbl, random_correct, band_fn)
                sync()
                # the root's part of a step is its own band's kernels (the rest of its step is
                # waiting for the peers); a peer's part is everything up to its last hand-over
                mine = self._compute_s if self.rank == 0 else time.perf_counter() - t0
        finally:
            self._time_compute = False
        nccl = str(dist_.get_backend(self.group)).lower() == "nccl"
        t = torch.tensor([mine], dtype=torch.float64, device=self.device if (on_gpu and nccl) else "cpu")
        times = [torch.zeros_like(t) for _ in range(self.world)]
        dist_.all_gather(times, t, group=self.group)
        times = [float(x.item()) for x in times]
        rates = [self.band_rows[r] / times[r] if (times[r] > 0 and self.band_rows[r] > 0) else 0.0
                 for r in range(self.world)]
        if not any(x > 0 for x in rates):
            return [b / max(self.total_rows, 1) for b in self.band_rows]
        # shares move at most 2x per call (one noisy measurement must not starve a rank: a tiny band's
        # rate is dominated by fixed costs and would not recover), and no rank drops below 1 %
        cur = [max(b / max(self.total_rows, 1), 1e-3) for b in self.band_rows]
        tgt = [x / sum(rates) for x in rates]
        new = [c * min(max(t / c, 0.5), 2.0) for c, t in zip(cur, tgt)]
        self.weights = [max(x / sum(new), 0.01) for x in new]
        self._layout(band_split_weighted(self.ref.n, self.n_qry, self.weights))
        return [b / max(self.total_rows, 1) for b in self.band_rows]


def query_sharded(ref, qry, kmers, random_tbl, rank, world_size, random_correct=True,
                  gather=True, band_fn=None, group=None):
    """Config 3/4 shape: every rank holds the full resident sketches, computes its band
    of query rows and (optionally) the bands are gathered into the PopPUNK-ordered
    matrix on rank 0.  `band_fn(q_begin, q_end) -> tensor` overrides the HIP launch
    (used by the CPU gloo tests to exercise the sharding/gather logic)."""
    n_qry = qry.n if qry is not None else 0
    bounds = shard_bounds(ref.n, n_qry, world_size)
    rows = [rows_in_band(ref.n, n_qry, bounds[i], bounds[i + 1]) for i in range(world_size)]
    qb, qe = bounds[rank], bounds[rank + 1]
    if band_fn is not None:
        local = band_fn(qb, qe)
    else:
        local, _ = dist(ref, qry, kmers, random_tbl, random_correct=random_correct, q_begin=qb,
                        q_end=qe)
    if not gather:
        return local, rows
    full = gather_bands(local, rows, local.shape[1], local.dtype, local.device, rank, world_size,
                        0, group)
    return full, rows


class _DeviceRows:
    """What `dist` asks of its `out` argument, over raw device memory (rows of a window another process owns)."""

    def __init__(self, ptr, rows, cols):
        self._ptr, self.shape = int(ptr), (int(rows), int(cols))

    def numel(self):
        return self.shape[0] * self.shape[1]

    def is_contiguous(self):
        return True

    def element_size(self):
        return 4

    def data_ptr(self):
        return self._ptr


class _WindowArray:
    """`__cuda_array_interface__` over a window: torch.as_tensor makes a tensor on it without a copy."""

    def __init__(self, ptr, rows, cols):
        self.__cuda_array_interface__ = {"shape": (int(rows), int(cols)), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class PeerStoreQuery:
    """The N-GPU distance job with NO transfer step ("peers write directly at final offsets via
    ... IPC"): the [n_pairs, 2] matrix is ONE device allocation on the root's GPU (`ppk_window_alloc`), every other
    rank of the node maps it (`ppk_window_export` / `ppk_window_open`: the 64-byte handle travels in one
    broadcast) and launches kernel 1 on its band with `out` = its rows of that window -- the float2 stores of its
    epilogue go over its own xGMI link into the root's HBM while the compare loop runs.  No send buffer, no
    receive, nothing on the data path but the kernel; a step ends with every rank's stream drained and one
    barrier, after which the root holds the whole PopPUNK-ordered matrix.

    UNVERIFIED ACROSS PHYSICAL DEVICES: the transport has run with two and four processes on ONE GPU only (no
    multi-GPU box on the builder's side); `run` therefore checks its first step against a gathered matrix and raises
    on a mismatch (see `run`, verify=).

    Bands are equal in pair count to begin with (a peer's 8 B per pair are far below what its link carries) and
    `rebalance` re-cuts them from measured per-rank times, like ShardedQuery's.  Collective calls: `open`, `run`,
    `rebalance`, `close`.  `open` raises RuntimeError ON EVERY RANK when any rank could not map the window
    (devices without peer access, processes that see different devices): the caller then uses ShardedQuery."""

    def __init__(self, ref, qry, rank, world_size, cols=2, group=None):
        self.ref, self.qry = ref, qry
        self.rank, self.world = int(rank), int(world_size)
        self.group = group
        self.cols = cols
        self.n_qry = qry.n if qry is not None else 0
        self.device = "cuda:%d" % ref.device
        self.window = None            # device pointer: the root's allocation, or this rank's mapping of it
        self.n_failed = None
        self._matrix = None
        self._verified = False        # run(verify="first") has checked this window against a gathered matrix
        self._set_bounds(shard_bounds(ref.n, self.n_qry, self.world))

    def _set_bounds(self, bounds):
        self.bounds = [int(b) for b in bounds]
        self.band_rows = [rows_in_band(self.ref.n, self.n_qry, self.bounds[r], self.bounds[r + 1])
                          for r in range(self.world)]
        self.band_off = [0]
        for r in range(self.world):
            self.band_off.append(self.band_off[-1] + self.band_rows[r])
        self.total_rows = self.band_off[-1]

    def flag_tensor(self, value):
        import torch.distributed as dist_
        torch = _torch()
        on_dev = self.world > 1 and str(dist_.get_backend(self.group)).lower() == "nccl"
        return torch.tensor([value], dtype=torch.int32, device=self.device if on_dev else "cpu")

    def open(self):
        import torch.distributed as dist_
        torch = _torch()
        lib = _lib.lib()
        nbytes = max(self.total_rows, 1) * self.cols * 4
        ok, why = 1, ""
        p = C.c_void_p()
        if self.rank == 0:
            rc = lib.ppk_window_alloc(self.ref.device, nbytes, C.byref(p))
            if rc != 0:
                ok, why = 0, _lib.last_error()
            else:
                self.window = p.value
        if self.world > 1:
            handle = C.create_string_buffer(64)
            if self.rank == 0 and ok:
                if lib.ppk_window_export(self.ref.device, self.window, handle) != 0:
                    ok, why = 0, _lib.last_error()
            t = self.flag_tensor(0).new_zeros(64, dtype=torch.uint8)
            if self.rank == 0:
                t.copy_(torch.frombuffer(bytearray(handle.raw), dtype=torch.uint8))
            dist_.broadcast(t, 0, group=self.group)
            if self.rank != 0:
                raw = bytes(t.cpu().numpy().tobytes())
                if not any(raw):
                    ok, why = 0, "the root exported no handle"
                elif lib.ppk_window_open(self.ref.device, raw, C.byref(p)) != 0:
                    ok, why = 0, _lib.last_error()
                else:
                    self.window = p.value
            flag = self.flag_tensor(ok)
            dist_.all_reduce(flag, op=dist_.ReduceOp.MIN, group=self.group)
            if int(flag.item()) == 0:
                self.close(collective=False)
                raise RuntimeError("PeerStoreQuery: the window could not be mapped on every rank" +
                                   (" (rank %d: %s)" % (self.rank, why) if why else ""))
        elif not ok:
            raise RuntimeError("PeerStoreQuery: " + why)
        if self.rank == 0:
            self._matrix = torch.as_tensor(_WindowArray(self.window, self.total_rows, self.cols), device=self.device)
        return self

    def matrix(self):
        """The whole matrix (rank 0; a tensor over the window, no copy)."""
        return self._matrix

    def _launch(self, kmers, random_tbl, random_correct):
        torch = _torch()
        rows = self.band_rows[self.rank]
        if rows == 0:
            return
        if self.n_failed is None:
            self.n_failed = torch.zeros(1, dtype=torch.int64, device=self.device)
        view = _DeviceRows(self.window + self.band_off[self.rank] * self.cols * 4, rows, self.cols)
        dist(self.ref, self.qry, kmers, random_tbl, random_correct=random_correct, q_begin=self.bounds[self.rank],
             q_end=self.bounds[self.rank + 1], out=view, n_failed=self.n_failed)

    def run(self, kmers=None, random_tbl=None, random_correct=True, verify="first", _fault=None):
        """One whole-job step; returns the matrix on rank 0 (None elsewhere) once EVERY rank's rows are in it.

        verify: "first" (default) -- the first step of this object checks the transport against an independent one:
        rank 0 fills the window with a sentinel, the step runs, every rank computes its band once more into a local
        buffer and those are gathered to rank 0 through `gather_bands` (send / recv), and the window must equal the
        gathered matrix bit for bit; RuntimeError on EVERY rank if it does not (the caller then uses ShardedQuery).
        "always": every step; None / False: never.  The default stays "first" until a run on two or more PHYSICAL
        GPUs has been recorded under profiles/ -- to date the peer stores have only crossed between two processes on
        one GPU (tests/test_gpu_multirank.py), never an xGMI link.  Collective when on."""
        import torch.distributed as dist_
        torch = _torch()
        if self.window is None:
            raise RuntimeError("PeerStoreQuery.run before open()")
        check = verify == "always" or (verify == "first" and not self._verified)
        if check:
            if self.rank == 0:
                self._matrix.view(torch.int32).fill_(0x7fc0dead)      # a NaN no distance is: a row that never arrives shows
                torch.cuda.current_stream(self.device).synchronize()
            if self.world > 1:
                dist_.barrier(self.group)
        self._launch(kmers, random_tbl, random_correct)
        torch.cuda.current_stream(self.device).synchronize()      # this rank's stores have left (kernel end = release)
        if self.world > 1:
            dist_.barrier(self.group)
            torch.cuda.current_stream(self.device).synchronize()
        if check:
            if _fault is not None:
                _fault(self)          # (tests: damage the window between the step and the check)
            self._check_against_gather(kmers, random_tbl, random_correct)
            self._verified = True
        return self._matrix if self.rank == 0 else None

    def _check_against_gather(self, kmers, random_tbl, random_correct):
        import torch.distributed as dist_
        torch = _torch()
        rows = self.band_rows[self.rank]
        local = torch.empty((max(rows, 1), self.cols), dtype=torch.float32, device=self.device)
        if rows:
            dist(self.ref, self.qry, kmers, random_tbl, random_correct=random_correct, q_begin=self.bounds[self.rank],
                 q_end=self.bounds[self.rank + 1], out=local[:rows])
        torch.cuda.current_stream(self.device).synchronize()
        if self.world > 1:
            whole = gather_bands(local[:rows], self.band_rows, self.cols, torch.float32, self.device, self.rank,
                                 self.world, dst=0, group=self.group)
        else:
            whole = local[:rows]
        ok = 1
        if self.rank == 0:
            ok = int(bool(torch.equal(whole.view(torch.int32), self._matrix.view(torch.int32))))
        if self.world > 1:
            flag = self.flag_tensor(ok)
            dist_.all_reduce(flag, op=dist_.ReduceOp.MIN, group=self.group)
            ok = int(flag.item())
        if not ok:
            raise RuntimeError("PeerStoreQuery: the matrix the ranks stored into the window differs from the gathered "
                               "one (peer stores are unverified across physical devices): use ShardedQuery")

    def rebalance(self, kmers=None, random_tbl=None, random_correct=True, steps=2):
        """Re-cut the bands in proportion to each rank's measured pairs per second (its kernel INCLUDING its stores
        into the window: a rank behind a slower link gets fewer rows).  Collective.  Returns the new shares."""
        import torch.distributed as dist_
        torch = _torch()
        if self.world == 1:
            return [1.0]
        for _ in range(max(1, steps)):
            dist_.barrier(self.group)
            torch.cuda.synchronize(self.device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
            self._launch(kmers, random_tbl, random_correct)
            e1.record(torch.cuda.current_stream(self.device))
            e1.synchronize()
            mine = max(e0.elapsed_time(e1), 1e-3)
            t = self.flag_tensor(0).new_zeros(self.world, dtype=torch.float32)
            t[self.rank] = self.band_rows[self.rank] / mine
            dist_.all_reduce(t, op=dist_.ReduceOp.SUM, group=self.group)
            rates = [max(float(x), 1e-9) for x in t.cpu().tolist()]
            self._set_bounds(band_split_weighted(self.ref.n, self.n_qry, rates))     # (the window is sized by the
            #                                                    pair space, not by the cut: nothing to re-allocate)
        dist_.barrier(self.group)
        return [b / max(self.total_rows, 1) for b in self.band_rows]

    def close(self, collective=True):
        import torch.distributed as dist_
        torch = _torch()
        lib = _lib.lib()
        if collective and self.world > 1:
            torch.cuda.synchronize(self.device)
            dist_.barrier(self.group)        # nobody is still storing into a window that is about to go
        self._matrix = None
        if self.window is not None and self.rank != 0:
            lib.ppk_window_close(self.ref.device, self.window)
            self.window = None
        if collective and self.world > 1:
            dist_.barrier(self.group)        # every mapping is gone before the allocation is
        if self.window is not None:
            lib.ppk_window_free(self.ref.device, self.window)
            self.window = None


def edges_sharded(ref, qry, kmers, random_tbl, rank, world_size, slope=2, x_max=0.0, y_max=0.0,
                  scale=(1.0, 1.0), inclusive=True, random_correct=True, band_fn=None, group=None,
                  device=None, cap=None):
    """BASELINE config 5 on N GPUs: every rank runs the fused distance -> boundary -> edge-list
    kernels on its band of query rows; only the edge lists move.  One all-gather of the per-rank
    edge counts, then the variable-length lists go to rank 0 with the same grouped send/recv as
    the distance blocks (`gather_bands`).  Bands are contiguous row ranges in rank order, so the
    concatenation is the edge list of the whole matrix in PopPUNK row order -- equal to
    `dist_edges` on one GPU.  Bands are equal here: an edge list is ~1e-3 of a distance block, so
    there is no transfer to balance.  Returns (edges int64 [n_edges, 2] on rank 0 / None
    elsewhere, per-rank edge counts).  `band_fn(q_begin, q_end) -> int64 [n, 2]` overrides the
    HIP launch (CPU gloo tests)."""
    torch = _torch()
    import torch.distributed as dist_
    n_qry = qry.n if qry is not None else 0
    bounds = shard_bounds(ref.n, n_qry, world_size)
    qb, qe = bounds[rank], bounds[rank + 1]
    if band_fn is not None:
        local = band_fn(qb, qe)
    elif qe > qb:
        local, _ = dist_edges(ref, qry, kmers, random_tbl, random_correct=random_correct, slope=slope,
                              x_max=x_max, y_max=y_max, scale=scale, inclusive=inclusive, q_begin=qb,
                              q_end=qe, cap=cap)
    else:
        local = torch.empty((0, 2), dtype=torch.int64, device=device or "cuda:%d" % ref.device)
    local = local.contiguous()
    if world_size == 1:
        return local, [int(local.shape[0])]
    nccl = str(dist_.get_backend(group)).lower() == "nccl"
    cnt = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device if nccl else "cpu")
    counts = [torch.zeros_like(cnt) for _ in range(world_size)]
    dist_.all_gather(counts, cnt, group=group)
    counts = [int(c.item()) for c in counts]
    full = gather_bands(local, counts, 2, torch.int64, local.device, rank, world_size, 0, group)
    return full, counts
