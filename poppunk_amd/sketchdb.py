"""Sketch database files for the distance engine.

The reference stores sketches in `<prefix>/<basename>.h5` with one uint64 dataset
per (sample, k) under /sketches/<name>/<k> and the attributes `sketchsize64`,
`bbits`, `kmers`, `length`, `missing_bases`, `base_freq` on the sample group,
`sketch_version`, `codon_phased` on /sketches (PopPUNK/web.py:14-61; readers
PopPUNK/sketchlib.py:109-214), plus the /random group that pp_sketchlib.addRandom
leaves there (PopPUNK/sketchlib.py:437-473; its presence is what PopPUNK checks,
:455-466).  Sketching itself is poppunk_amd/sketching.py (pp_sketchlib.constructDatabase); what it
writes through save_h5 carries sketch_version "poppunk_amd:sketch1" [EXT: not pp-sketchlib's rule].

Two on-disk forms are read and written here:

  `<db>.h5`   the reference's layout, through poppunk_amd.h5lite (libhdf5 via ctypes) or h5py,
              whichever the interpreter has;
  `<db>.npz`  the same content flat (fast to load; what the synthetic benchmarks use):
                names str [n] | kmers int32 [nk] | sketches uint64 [n, nk, sketchsize64*bbits]
                sketchsize64, bbits int | lengths int64 [n], base_freq float64 [n, 4] (optional)
                random_table float32 [nk, n_clu, n_clu], clusters uint16 [n] (optional)
                random/<dataset>, random@<attribute>: the /random group's raw content, verbatim

The /random group [EXT].  Its internal layout belongs to pp-sketchlib and is not stated anywhere
in the reference tree.  The layout recalled from pp-sketchlib's database code is
    table_keys (sample names) / table_values (uint16 cluster of each) -- "save_hash" pairs
    matches_keys (k-mer lengths) / matches_values (per k an n_clu x n_clu matrix)
    centroids (n_clu x 4 base frequencies), attributes k_min, k_max, use_rc
`random_from_raw` maps exactly that (and nothing looser) to the engine's `random_table` /
`clusters`; a group it does not recognise is carried through conversions verbatim and reported,
never silently dropped: `pp_sketchlib.queryDatabase(random_correct=True)` then raises unless the
caller opts out (see there).
"""
import os
import sys

import numpy as np


def _h5_backend():
    """('h5lite' | 'h5py', open(path, mode)) -- h5py when the interpreter has it, else libhdf5."""
    try:
        import h5py
        return "h5py", (lambda path, mode="r": h5py.File(path, mode))
    except ImportError:
        pass
    from . import h5lite
    if h5lite.available():
        return "h5lite", (lambda path, mode="r": h5lite.File(path, mode))
    raise ImportError("neither h5py nor libhdf5 (set HDF5_LIB) is available")


def _ds_read(obj):
    return obj.read() if hasattr(obj, "read") else obj[()]


def _is_group(obj):
    return hasattr(obj, "keys")


def db_file(prefix, ext):
    return prefix + ext


class LoadedSketches:
    def __init__(self, names, kmers, sketches, sketchsize64, bbits, random_table, clusters,
                 random_raw=None, lengths=None, base_freq=None, random_status="absent", missing_bases=None):
        self.names = names
        self.kmers = kmers
        self.sketches = sketches
        self.sketchsize64 = sketchsize64
        self.bbits = bbits
        self.random_table = random_table
        self.clusters = clusters
        self.random_raw = random_raw          # {"name": array, "@attr": value}: the /random group as found
        self.lengths = lengths
        self.base_freq = base_freq
        # "absent" | "mapped" ([EXT] layout recognised) | "unrecognised" (present, carried raw only)
        self.random_status = random_status
        self.missing_bases = missing_bases    # int64 [n] ambiguous-base counts, None where the file has none


def _select_kmers(db_kmers, klist):
    db_kmers = [int(k) for k in db_kmers]
    idx = []
    for k in klist:
        if int(k) not in db_kmers:
            raise RuntimeError("k-mer length %d not found in sketch database (has %s)"
                               % (int(k), db_kmers))
        idx.append(db_kmers.index(int(k)))
    return idx


# ---- the /random group -----------------------------------------------------------------------

def read_random_raw(grp):
    """Every dataset and attribute of a /random group, by name, as numpy values (generic walk:
    nothing is assumed about the layout).  Nested groups are flattened with '/' in the key."""
    raw = {}

    def visit(g, prefix):
        for a in list(g.attrs.keys()):
            raw["@" + prefix + a] = np.asarray(g.attrs[a])
        for name in list(g.keys()):
            obj = g[name]
            if _is_group(obj):
                visit(obj, prefix + name + "/")
            else:
                raw[prefix + name] = np.asarray(_ds_read(obj))
    visit(grp, "")
    return raw


def random_from_raw(raw, names, klist, base_freq=None):
    """[EXT] Map the recalled pp-sketchlib /random layout (module docstring) to
    (random_table float32 [nk, C, C], clusters uint16 [n]); None when `raw` is not exactly that.
    Samples absent from the cluster table (queries from another database) take the cluster whose
    centroid is nearest to their base frequencies [EXT closest_cluster], or cluster 0 when the
    frequencies are unknown.  k outside [k_min, k_max]: random match chance 1 below, 0 above [EXT]."""
    need = ("table_keys", "table_values", "matches_keys", "matches_values")
    if raw is None or any(k not in raw for k in need):
        return None
    tk = np.asarray(raw["table_keys"]).ravel()
    try:
        # (one C-level conversion for the common fixed-length byte strings; anything else name by name)
        keys = tk.astype(str).tolist() if tk.dtype.kind in "SU" else None
    except (UnicodeDecodeError, ValueError):
        keys = None
    if keys is None:
        keys = [x.decode("utf-8", "replace") if isinstance(x, bytes) else str(x) for x in tk]
    vals = np.asarray(raw["table_values"]).ravel()
    mk = [int(x) for x in np.asarray(raw["matches_keys"]).ravel()]
    mv = np.asarray(raw["matches_values"], dtype=np.float64)
    if len(keys) != len(vals) or mv.shape[0] != len(mk) or len(mk) == 0:
        return None
    per = int(np.prod(mv.shape[1:])) if mv.ndim > 1 else 0
    n_clu = int(round(per ** 0.5))
    if n_clu < 1 or n_clu * n_clu != per or (len(vals) and int(vals.max()) >= n_clu):
        return None
    mv = mv.reshape(len(mk), n_clu, n_clu)
    k_min = int(np.asarray(raw.get("@k_min", min(mk))).ravel()[0])
    k_max = int(np.asarray(raw.get("@k_max", max(mk))).ravel()[0])
    tbl = np.empty((len(klist), n_clu, n_clu), dtype=np.float32)
    for i, k in enumerate(klist):
        if int(k) in mk:
            tbl[i] = mv[mk.index(int(k))]
        elif int(k) < k_min:
            tbl[i] = 1.0
        elif int(k) > k_max:
            tbl[i] = 0.0
        else:
            return None
    cent = np.asarray(raw["centroids"], dtype=np.float64) if "centroids" in raw else None
    if cent is not None and (cent.ndim != 2 or cent.shape[0] != n_clu):
        cent = None
    if list(names) == keys:                       # the table lists exactly these samples in this order
        return tbl, np.ascontiguousarray(vals, dtype=np.uint16)
    of = dict(zip(keys, vals.tolist()))
    found = np.fromiter((of.get(nm, -1) for nm in names), dtype=np.int64, count=len(names))
    clusters = np.where(found >= 0, found, 0).astype(np.uint16)
    absent = np.flatnonzero(found < 0)
    if absent.size and cent is not None and base_freq is not None and cent.shape[1] == np.asarray(base_freq).shape[1]:
        bf = np.asarray(base_freq, dtype=np.float64)[absent]
        clusters[absent] = np.argmin(((cent[None, :, :] - bf[:, None, :]) ** 2).sum(axis=2), axis=1).astype(np.uint16)
    return tbl, clusters


def random_to_raw(random_table, clusters, names, kmers):
    """The inverse, for the writer: (random_table, clusters) in the recalled layout [EXT]."""
    tbl = np.asarray(random_table, dtype=np.float64)
    n_clu = tbl.shape[1]
    return {"table_keys": np.asarray([str(n).encode() for n in names]),
            "table_values": np.asarray(clusters if clusters is not None else np.zeros(len(names)), dtype=np.uint16),
            "matches_keys": np.asarray(kmers, dtype=np.uint64),
            "matches_values": tbl.reshape(len(kmers), n_clu * n_clu),
            "@k_min": np.uint32(min(kmers)), "@k_max": np.uint32(max(kmers)), "@use_rc": np.uint8(1)}


def reads_flags(path, names):
    """The per-sample `reads` flags of the database file `path` (.npz or .h5) in the order of `names`, or None when
    the file stores none."""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            if "reads" not in z.files:
                return None
            pos = {str(nm): i for i, nm in enumerate(z["names"])}
            return [bool(z["reads"][pos[str(nm)]]) for nm in names]
    f = _h5_backend()[1](path, "r")
    try:
        top = f["sketches"]
        flags = []
        for nm in names:
            attrs = top[str(nm)].attrs
            flags.append(bool(np.asarray(attrs["reads"]).ravel()[0]) if "reads" in list(attrs.keys()) else None)
        return None if all(x is None for x in flags) else [bool(x) for x in flags]
    finally:
        f.close()


# ---- .npz ---------------------------------------------------------------------------------------

def save_npz(db_name, names, kmers, sketches, sketchsize64, bbits, random_table=None,
             clusters=None, random_raw=None, lengths=None, base_freq=None, missing_bases=None, reads=None):
    """db_name is the reference's `<prefix>/<basename>` (no extension).  reads: per sample, whether it was sketched
    from reads (stored only when given)."""
    os.makedirs(os.path.dirname(db_name) or ".", exist_ok=True)
    payload = dict(names=np.asarray(names, dtype=str), kmers=np.asarray(kmers, dtype=np.int32),
                   sketches=np.ascontiguousarray(sketches, dtype=np.uint64),
                   sketchsize64=np.int32(sketchsize64), bbits=np.int32(bbits))
    if random_table is not None:
        payload["random_table"] = np.asarray(random_table, dtype=np.float32)
    if clusters is not None:
        payload["clusters"] = np.asarray(clusters, dtype=np.uint16)
    if lengths is not None:
        payload["lengths"] = np.asarray(lengths, dtype=np.int64)
    if base_freq is not None:
        payload["base_freq"] = np.asarray(base_freq, dtype=np.float64)
    if missing_bases is not None:
        payload["missing_bases"] = np.asarray(missing_bases, dtype=np.int64)
    if reads is not None:
        payload["reads"] = np.asarray(reads, dtype=np.uint8)
    for key, val in (random_raw or {}).items():
        val = np.asarray(val)
        if val.dtype == object:
            val = val.astype(str)
        payload[("random@" + key[1:]) if key.startswith("@") else ("random/" + key)] = val
    np.savez(db_name + ".npz", **payload)


def _load_npz(path, names, klist):
    with np.load(path, allow_pickle=False) as z:
        db_names = [str(x) for x in z["names"]]
        pos = {nm: i for i, nm in enumerate(db_names)}
        missing = [nm for nm in names if nm not in pos]
        if missing:
            raise RuntimeError("samples not found in sketch database %s: %s"
                               % (path, ", ".join(missing[:5])))
        kidx = _select_kmers(z["kmers"], klist)
        rows = np.asarray([pos[nm] for nm in names], dtype=np.int64)
        sk = z["sketches"][rows][:, kidx, :]
        raw = {}
        for key in z.files:
            if key.startswith("random/"):
                raw[key[len("random/"):]] = z[key]
            elif key.startswith("random@"):
                raw["@" + key[len("random@"):]] = z[key]
        lengths = z["lengths"][rows] if "lengths" in z.files else None
        base_freq = z["base_freq"][rows] if "base_freq" in z.files else None
        missing = z["missing_bases"][rows] if "missing_bases" in z.files else None
        tbl = z["random_table"][kidx] if "random_table" in z.files else None
        clu = z["clusters"][rows] if "clusters" in z.files else None
        status = "mapped" if tbl is not None else "absent"
        if tbl is None and raw:
            mapped = random_from_raw(raw, names, klist, base_freq)
            if mapped is not None:
                tbl, clu = mapped
                status = "mapped"
            else:
                status = "unrecognised"
        return LoadedSketches(list(names), np.asarray(klist, dtype=np.int32),
                              np.ascontiguousarray(sk), int(z["sketchsize64"]), int(z["bbits"]),
                              tbl, clu, raw or None, lengths, base_freq, status, missing)


# ---- .h5 ------------------------------------------------------------------------------------------

def _random_of_file(path):
    """The /random group's raw content ({} when it has no datasets), through h5py or libhdf5."""
    _, h5open = _h5_backend()
    f = h5open(path, "r")
    try:
        return read_random_raw(f["random"]) if "random" in f else None
    finally:
        f.close()


def _finish_h5(names, klist, sk, s64, bbits, lengths, base_freq, raw, missing=None):
    have_freq = base_freq is not None and not np.isnan(base_freq).any()
    tbl, clu, status = None, None, "absent"
    if raw is not None:
        mapped = random_from_raw(raw, names, klist, base_freq if have_freq else None)
        if mapped is not None:
            tbl, clu = mapped
            status = "mapped"
        else:
            status = "unrecognised"
    return LoadedSketches(list(names), np.asarray(klist, dtype=np.int32), sk, s64, bbits, tbl, clu, raw,
                          lengths, base_freq if have_freq else None, status,
                          None if missing is None else np.asarray(missing))


def _pick(path, file_names, file_kmers, names, klist):
    """Row and k indices of a request in a whole-file image (None, None = the image as it is)."""
    kidx = [file_kmers.index(int(k)) for k in klist]
    if names == file_names and kidx == list(range(len(file_kmers))):
        return None, None
    pos = {nm: i for i, nm in enumerate(file_names)}
    rows = np.empty(len(names), dtype=np.int64)
    for i, nm in enumerate(names):
        r = pos.get(nm)
        if r is None:
            raise RuntimeError("sample %s not found in sketch database %s" % (nm, path))
        rows[i] = r
    return rows, kidx


def _take(a, rows, kidx=None):
    if a is None or rows is None:
        return a
    a = a[rows]
    return np.ascontiguousarray(a[:, kidx]) if kidx is not None else a


# what the last _load_h5 did: {"source": "sidecar" | "h5", "backend": 1 direct reader | 2 libhdf5,
# "packed": a sidecar was written, "declined": why the direct reader passed the file on}
last_load = {}


def _load_h5(path, names, klist):
    """`names` x `klist` from a reference-layout `.h5` (PopPUNK/web.py:14-61): from its packed sidecar when
    there is a valid one (poppunk_amd/h5bulk.py), else ONE native bulk read (`ppk_h5_read`, include/ppk.h)
    -- which packs the whole file into the sidecar when the request covers at least half of it."""
    from . import h5bulk
    if len(names) == 0:
        raise RuntimeError("no sample names given")
    names = list(names)
    klist = [int(k) for k in klist]
    last_load.clear()
    side = h5bulk.sidecar_open(path)
    if side is not None and all(k in side.kmers for k in klist):
        rows, kidx = _pick(path, side.names, side.kmers, names, klist)
        raw = side.random_raw
        if side.has_random and raw is None:
            raw = {}
        last_load.update(source="sidecar", backend=0, packed=False, declined="")
        return _finish_h5(names, klist, _take(side.sketches, rows, kidx), side.sketchsize64, side.bbits,
                          np.asarray(_take(side.lengths, rows)), _take(side.base_freq, rows), raw,
                          _take(np.asarray(side.missing), rows))
    stamp = h5bulk.h5_stamp(path)
    with h5bulk.H5Bulk(path) as f:
        s64, bbits, _ = f.params()
        words = s64 * bbits
        pack = h5bulk.sidecar_enabled() and 2 * len(names) >= f.count()
        want = f.names() if pack else names
        try:
            sk, lengths, missing, freq = f.read(want, klist, words)
        except RuntimeError:
            if not pack:
                raise
            pack = False                      # e.g. a k-mer length only some samples have: read what was asked
            sk, lengths, missing, freq = f.read(names, klist, words)
        raw = _random_of_file(path) if f.has_random else None
        last_load.update(source="h5", backend=f.backend, packed=False, declined=f.declined)
    if not pack:
        return _finish_h5(names, klist, sk, s64, bbits, lengths, freq, raw, missing)
    # (base_freq rows of samples without the attribute are NaN in the image too: whether a request has the
    # frequencies is decided over the rows it selects, _finish_h5, exactly as on the direct read)
    last_load["packed"] = h5bulk.sidecar_write(path, stamp, want, klist, sk, s64, bbits, lengths, missing,
                                               freq, raw is not None, raw)
    rows, _ = _pick(path, want, klist, names, klist)
    return _finish_h5(names, klist, _take(sk, rows), s64, bbits, _take(lengths, rows), _take(freq, rows), raw,
                      _take(np.asarray(missing), rows))


def save_h5(db_name, names, kmers, sketches, sketchsize64, bbits, random_table=None, clusters=None,
            random_raw=None, lengths=None, base_freq=None, sketch_version="poppunk_amd", codon_phased=False,
            missing_bases=None, reads=None):
    """Write `<db_name>.h5` in the reference's layout (PopPUNK/web.py:14-61 for /sketches; attribute
    names as its readers use them, PopPUNK/sketchlib.py:124-133,155-158).  /random: `random_raw`
    verbatim when given (a round trip of what a conversion carried), else (random_table, clusters)
    in the recalled pp-sketchlib layout [EXT].  reads: per sample, whether it was sketched from reads -- the `reads`
    attribute qc.sketchlibAssemblyQC looks for, written only when given."""
    _, h5open = _h5_backend()
    os.makedirs(os.path.dirname(db_name) or ".", exist_ok=True)
    sketches = np.ascontiguousarray(sketches, dtype=np.uint64)
    kmers = [int(k) for k in kmers]
    f = h5open(db_name + ".h5", "w")
    try:
        top = f.create_group("sketches")
        top.attrs["sketch_version"] = str(sketch_version)
        top.attrs["codon_phased"] = bool(codon_phased)
        for i, nm in enumerate(names):
            g = top.create_group(str(nm))
            g.attrs["sketchsize64"] = np.int64(sketchsize64)
            g.attrs["bbits"] = np.int64(bbits)
            g.attrs["kmers"] = np.asarray(kmers, dtype=np.int64)
            g.attrs["length"] = np.int64(lengths[i] if lengths is not None else 0)
            g.attrs["missing_bases"] = np.int64(missing_bases[i] if missing_bases is not None else 0)
            if reads is not None:
                g.attrs["reads"] = bool(reads[i])
            bf = np.asarray(base_freq[i] if base_freq is not None else [0.25] * 4, dtype=np.float64)
            if not np.isnan(bf).any():        # a NaN row = a sample that had no base_freq attribute: it gets none
                g.attrs["base_freq"] = bf
            for j, k in enumerate(kmers):
                d = g.create_dataset(str(k), data=sketches[i, j])
                d.attrs["kmer-size"] = np.int64(k)
        if random_raw is None and random_table is not None:
            random_raw = random_to_raw(random_table, clusters, names, kmers)
        if random_raw:
            groups = {"": f.create_group("random")}

            def group_of(path):
                if path not in groups:
                    parent, _, leaf = path.rpartition("/")
                    groups[path] = group_of(parent).create_group(leaf)
                return groups[path]

            for key, val in random_raw.items():
                is_attr = key.startswith("@")
                path, _, leaf = (key[1:] if is_attr else key).rpartition("/")
                g = group_of(path)
                val = np.asarray(val)
                if val.dtype.kind in "UO" or (val.dtype.kind == "S" and is_attr):
                    val = np.asarray([x if isinstance(x, bytes) else str(x).encode() for x in val.ravel()]).reshape(val.shape)
                if is_attr:
                    g.attrs[leaf] = val.item().decode() if val.dtype.kind == "S" and val.ndim == 0 else val
                else:
                    # (name lists: fixed-length byte strings, as HighFive / h5py store them)
                    g.create_dataset(leaf, data=val)
    finally:
        f.close()


def convert_h5_to_npz(db_name, out_name=None):
    """Rewrite the reference's `<db_name>.h5` as `<out_name>.npz` (default: next to it) with every
    sample and every k-mer length it holds, the per-sample `length` / `base_freq`, and the /random
    group: its raw datasets verbatim (`random/...`, `random@...`) and -- when the [EXT] layout is
    recognised -- the mapped `random_table` / `clusters`.  Returns (n_samples, kmers, random status)."""
    _, h5open = _h5_backend()
    f = h5open(db_name + ".h5", "r")
    try:
        grp = f["sketches"]
        names = sorted(grp.keys())
        if not names:
            raise RuntimeError("no samples in %s.h5" % db_name)
        kmers = sorted(int(k) for k in np.asarray(grp[names[0]].attrs["kmers"]).ravel())
    finally:
        f.close()
    loaded = _load_h5(db_name + ".h5", names, kmers)
    save_npz(out_name or db_name, loaded.names, loaded.kmers, loaded.sketches, loaded.sketchsize64,
             loaded.bbits, loaded.random_table, loaded.clusters, loaded.random_raw, loaded.lengths,
             loaded.base_freq)
    if loaded.random_status == "unrecognised":
        sys.stderr.write("poppunk_amd: the /random group of %s.h5 is not in the layout this package knows; its "
                         "datasets (%s) are carried into the .npz verbatim under random/...\n"
                         % (db_name, ", ".join(sorted(k for k in loaded.random_raw))))
    return len(names), kmers, loaded.random_status


def load(db_name, names, klist):
    """Load `names` x `klist` from `<db_name>.npz` (preferred) or `<db_name>.h5`."""
    names = [str(n) for n in names]
    klist = [int(k) for k in np.asarray(klist).ravel()]
    if len(names) == 0:
        raise RuntimeError("no sample names given")
    if os.path.exists(db_name + ".npz"):
        return _load_npz(db_name + ".npz", names, klist)
    if os.path.exists(db_name + ".h5"):
        try:
            return _load_h5(db_name + ".h5", names, klist)
        except ImportError:
            raise RuntimeError("reading %s.h5 needs h5py or libhdf5 (HDF5_LIB=/path/to/libhdf5.so), neither is "
                               "available; convert the database with `python -m poppunk_amd.sketchdb %s` in an "
                               "interpreter that has one" % (db_name, db_name))
    raise RuntimeError("sketch database %s(.npz|.h5) not found" % db_name)


# ---- database parameter readers (PopPUNK/sketchlib.py:109-214) ------------------------------------

def getSeqsInDb(dbname):
    """Sample names in a sketch database file (PopPUNK/sketchlib.py:197-214); `.h5` or `.npz`."""
    if dbname.endswith(".npz"):
        with np.load(dbname, allow_pickle=False) as z:
            return [str(x) for x in z["names"]]
    from . import h5bulk
    with h5bulk.H5Bulk(dbname) as f:
        return f.names()


def _checked_params(path, dbPrefix, what):
    """One native pass over every sample's sketchsize64 / kmers attributes with the reference's consistency
    checks (PopPUNK/sketchlib.py:109-168: a message on stderr and `sys.exit(1)` on a mixed database).
    Returns (sorted kmers of the first sample, its sketchsize64, codon_phased)."""
    from . import h5bulk
    with h5bulk.H5Bulk(path) as f:
        if f.count() == 0:
            # getKmersFromReferenceDatabase returns an empty array for a database without samples
            # (PopPUNK/sketchlib.py:154-168); only readDBParams turns that into the message and the exit (:188-191)
            if what == "both":
                sys.stderr.write("Couldn't find sketches in " + dbPrefix + "\n")
                sys.exit(1)
            return [], 0, bool(f.codon_phased)
        s64, _, km, nk = f.all_params()
        names = f.names()          # (after the pass: a reader hand-over inside it changes the listing)
        phased = bool(f.codon_phased)
    first = [int(k) for k in km[0, :int(nk[0])]]
    if what in ("kmers", "both"):
        same = (nk == nk[0]) & (km[:, :int(nk[0])] == km[0, :int(nk[0])]).all(axis=1)
        if what == "both":                      # readDBParams compares the sorted lists
            same = (nk == nk[0]) & (np.sort(km[:, :int(nk[0])], axis=1) == np.sort(km[0, :int(nk[0])])).all(axis=1)
        if not same.all():
            bad = int(np.flatnonzero(~same)[0])
            ks = [int(k) for k in km[bad, :min(int(nk[bad]), km.shape[1])]]
            ref = first
            if what == "both":
                ks, ref = sorted(ks), sorted(first)
            sys.stderr.write("Problem with database; kmer lengths inconsistent: %s vs %s\n" % (ks, ref))
            sys.exit(1)
    if what in ("size", "both"):
        diff = np.flatnonzero(s64 != s64[0])
        if diff.size:
            bad = int(diff[0])
            sys.stderr.write("Problem with database; sketch sizes for sample %s is %d, but smaller kmers "
                             "have sketch sizes of %d\n" % (names[bad], int(s64[0]), int(s64[bad])))
            sys.exit(1)
    return first, int(s64[0]), phased


def readDBParams(dbPrefix):
    """(kmers, sketch size in units of 64 bins, codon_phased) of `<dbPrefix>/<basename>.h5|.npz`
    (PopPUNK/sketchlib.py:170-195, with the consistency checks of :109-168)."""
    base = dbPrefix + "/" + os.path.basename(dbPrefix)
    if os.path.exists(base + ".h5"):
        ks, s64, phased = _checked_params(base + ".h5", dbPrefix, "both")
        return np.asarray(sorted(ks)), s64, phased
    with np.load(base + ".npz", allow_pickle=False) as z:
        return np.sort(np.asarray(z["kmers"], dtype=np.int64)), int(z["sketchsize64"]), False


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit("usage: python -m poppunk_amd.sketchdb <prefix>/<basename> [<out prefix>/<basename>]   (.h5 -> .npz)")
    n_done, k_done, r_done = convert_h5_to_npz(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else None)
    print("wrote %s.npz: %d samples, k = %s, /random: %s"
          % (sys.argv[2] if len(sys.argv) == 3 else sys.argv[1], n_done, k_done, r_done))


# ---- database files either side of the distance call: --update-db, QC pruning, reference picking -------

def _prefix_file(prefix, suffix=".h5"):
    return prefix + "/" + os.path.basename(prefix) + suffix


def getSketchSize(dbPrefix):
    """(sketch size in units of 64 bins, codon_phased), checked for consistency over the samples
    (PopPUNK/sketchlib.py:109-142; `sys.exit(1)` on a mixed database)."""
    _, s64, phased = _checked_params(_prefix_file(dbPrefix), dbPrefix, "size")
    return int(s64), phased


def getKmersFromReferenceDatabase(dbPrefix):
    """Sorted k-mer lengths of the database, checked for consistency (PopPUNK/sketchlib.py:144-168)."""
    ks, _, _ = _checked_params(_prefix_file(dbPrefix), dbPrefix, "kmers")
    return np.asarray(sorted(ks))


def get_database_statistics(prefix):
    """(genome lengths, ambiguous-base counts) per sample in database order
    (PopPUNK/sketchlib.py:672-690; callers PopPUNK/__main__.py:404,:492 for QC)."""
    from . import h5bulk
    path = _prefix_file(prefix)
    side = h5bulk.sidecar_open(path)
    if side is not None:
        return list(side.lengths), list(side.missing)
    with h5bulk.H5Bulk(path) as f:
        names = f.names()
        if not names:
            return [], []
        s64, bbits, ks = f.params()
        _, lengths, missing, _ = f.read(names, ks[:1], s64 * bbits)
    return list(lengths), list(missing)


def _copy_samples(src_sketches, dst_sketches, skip=frozenset()):
    """Every sample group of `src_sketches` that is not in `skip` -> `dst_sketches`, by the library's object copy
    (datasets and attributes as stored).  Returns (copied, skipped) name lists; the name being copied when the
    library refuses is left in `_copy_samples.current` for the caller's message."""
    copied, skipped = [], []
    for name in src_sketches.keys():
        _copy_samples.current = name
        if name in skip:
            skipped.append(name)
        else:
            dst_sketches.copy(src_sketches[name], name)
            copied.append(name)
    return copied, skipped


_copy_samples.current = ""


def joinDBs(db1, db2, output, update_random=None, full_names=False):
    """The sketches of two databases in one file (PopPUNK/sketchlib.py:216-293; callers PopPUNK/assign.py:741,
    PopPUNK/visualise.py:493): db1's /sketches group whole, db2's samples added to it one by one, written as
    `<output>.tmp.h5` and renamed when complete (the output may be one of the inputs).

    /random: db1's group is carried over, as the reference does when `update_random` is None.  With
    `update_random` given the reference re-runs pp_sketchlib.addRandom on the joined file; sketching-side
    functions are outside this package (sketching is out of scope), so db1's table is
    carried here too and a line on stderr says so -- a sample absent from the table takes the nearest
    base-frequency cluster when it is queried (`random_from_raw`)."""
    first, second = (db1, db2) if full_names else (_prefix_file(db1), _prefix_file(db2))
    target = output if full_names else output + "/" + os.path.basename(output)
    _, h5open = _h5_backend()
    files = []
    try:
        try:
            for path, mode in ((first, "r"), (second, "r"), (target + ".tmp.h5", "w")):
                files.append(h5open(path, mode))
            src1, src2, dst = files
            src1.copy("sketches", dst)
            _copy_samples(src2["sketches"], dst["sketches"])
            if "random" in src1:
                src1.copy("random", dst)
            if update_random is not None:
                sys.stderr.write("poppunk_amd: random match chances of %s carried over to the joined database "
                                 "(not re-estimated: run pp_sketchlib.addRandom on it for that)\n" % first)
        finally:
            for f in files:
                f.close()
    except RuntimeError as e:
        sys.stderr.write("ERROR: " + str(e) + "\n")
        sys.stderr.write("Joining sketches failed, try running without --update-db\n")
        sys.exit(1)
    os.rename(target + ".tmp.h5", target + ".h5")


def removeFromDB(db_name, out_name, removeSeqs, full_names=False):
    """A copy of the database without the named samples (PopPUNK/sketchlib.py:296-346; callers
    PopPUNK/assign.py:800, PopPUNK/qc.py:515-525, PopPUNK/reference_pick.py:104).  As in the reference the
    prefix form writes `<out_name>/<basename>.tmp.h5` and leaves the rename to the caller; /random and the
    attributes of /sketches are kept; names that are not in the database are reported on stderr."""
    unwanted = frozenset(removeSeqs)
    source = db_name if full_names else _prefix_file(db_name)
    target = out_name if full_names else _prefix_file(out_name, ".tmp.h5")
    _, h5open = _h5_backend()
    dropped = []
    files = []
    try:
        try:
            files.append(h5open(source, "r"))
            files.append(h5open(target, "w"))
            src, dst = files
            if "random" in src:
                src.copy("random", dst)
            kept_group = dst.create_group("sketches")
            for key, value in src["sketches"].attrs.items():
                kept_group.attrs.create(key, value)
            _, dropped = _copy_samples(src["sketches"], kept_group, unwanted)
        finally:
            for f in files:
                f.close()
    except RuntimeError as e:
        sys.stderr.write("ERROR: " + str(e) + "\n")
        sys.stderr.write("Error while deleting sequence " + _copy_samples.current + "\n")
        sys.exit(1)
    not_found = unwanted.difference(dropped)
    if not_found:
        sys.stderr.write("WARNING: Did not find samples to remove:\n")
        sys.stderr.write("\t".join(not_found) + "\n")
