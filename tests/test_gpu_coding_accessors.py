"""A database without any coded copy (option "rank_planes" 0 at creation): every accessor of the coded copies answers
as it always has -- PPK_ERR_STATE with its own message, or 0 from the getters.  The messages are one table of four
nouns behind five shared helpers (ppk_coding.hip); this pins the table."""
import ctypes as C

import numpy as np
import pytest

from poppunk_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

NO_CODING = {
    "ppk_db_rank_read": "the database has no rank-coded copy",
    "ppk_db_rank_block_planes": "the database has no rank-coded copy",
    "ppk_db_fold_read": "the database has no folded pair",
    "ppk_db_fold_block_planes": "the database has no folded pair",
    "ppk_db_fold2_read": "the database has no two-holder pair",
    "ppk_db_fold2_block_planes": "the database has no two-holder pair",
    "ppk_db_fold2_stream_planes": "the database has no two-holder pair",
    "ppk_db_fold2_position_order": "the database has no two-holder pair",
    "ppk_db_fold2_events_read": "the database has no two-holder pair",
    "ppk_db_foldh_read": "the database has no holder pair",
    "ppk_db_foldh_stream_planes": "the database has no holder pair",
    "ppk_db_foldh_position_order": "the database has no holder pair",
    "ppk_db_foldh_entries_read": "the database has no holder pair",
}


def test_every_accessor_of_a_database_without_codings(ppk_option):
    n, s64, kmers = 64, 2, (13, 17, 21, 25, 29)
    ppk_option("rank_planes", 0)
    db = engine.SketchDB(synth.make_sketches(n, kmers=kmers, sketchsize64=s64)[0], s64, 14)
    ppk_option("rank_planes", 1)      # (read at creation: the accessors answer for the database, not the option)
    lib, h = _lib.lib(), db._h
    buf = np.zeros(1 << 16, dtype=np.uint64)
    p, cap = C.c_void_p(buf.ctypes.data), 1 << 16
    calls = {
        "ppk_db_rank_read": (h, p, cap), "ppk_db_rank_block_planes": (h, p, cap),
        "ppk_db_fold_read": (h, 0, p, cap), "ppk_db_fold_block_planes": (h, p, cap),
        "ppk_db_fold2_read": (h, 1, p, cap), "ppk_db_fold2_block_planes": (h, p, cap),
        "ppk_db_fold2_stream_planes": (h, p, cap), "ppk_db_fold2_position_order": (h, p, cap),
        "ppk_db_fold2_events_read": (h, p, 1, p, 0),
        "ppk_db_foldh_read": (h, 0, p, cap), "ppk_db_foldh_stream_planes": (h, p, cap),
        "ppk_db_foldh_position_order": (h, p, cap), "ppk_db_foldh_entries_read": (h, p, 1, p, 0),
    }
    assert set(calls) == set(NO_CODING)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == _lib.ERR_STATE, name
        assert lib.ppk_last_error().decode() == "%s: %s" % (name, NO_CODING[name])
    assert not buf.any()
    # the getters: no planes, no H, no list, no buckets, no count pass
    assert (db.rank_planes, db.fold_planes, db.fold2_planes, db.foldh_holders()) == (0, 0, 0, 0)
    for name in ("ppk_db_fold2_events", "ppk_db_foldh_entries"):
        nb = C.c_size_t(7)
        assert getattr(lib, name)(h, C.byref(nb)) == 0 and nb.value == 0
    assert lib.ppk_db_rank_counts(h, None, 0) == 0 and db.rank_counts() is None
    db.close()
