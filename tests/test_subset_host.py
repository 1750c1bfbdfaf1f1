"""CPU checks of the row-set interface (gsim_rowset_*, gsim_db_search_rows): the symbols exist, the stats struct matches the
header, and every argument error is reported before any device state -- on a table that is not on a GPU -- with a message and
with *out cleared.  A table that is not on a GPU is a state error, after the argument checks; never a host computation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gsim_rowset_from_rows", "gsim_rowset_from_bitmap", "gsim_rowset_count", "gsim_rowset_rows", "gsim_rowset_destroy",
           "gsim_db_search_rows"]
INVALID, STATE = -1, -5
BASE = 1000


def u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def table40():
    t = capi.Table(1024).add_rows(np.arange(40 * 32, dtype=np.uint32).reshape(40, 32))
    t.set_row_base(BASE)
    return t


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in capi.EXPORTS, s
    assert capi.GsimRowsetStats and capi.RowSet and capi.Table.rowset and capi.Table.search_rows


def test_stats_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_rowset_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == 6 and len(fields) == len(re.findall(r";", body)), "all uint64_t or double, as gsim_join_stats"
    assert [n for _, n in fields] == [n for n, _ in capi.GsimRowsetStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimRowsetStats._fields_]
    assert C.sizeof(capi.GsimRowsetStats) == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_ROWSET_EXCLUDE\s+1u", text)


def test_constructor_argument_errors_come_before_any_device_state():
    L = capi.load()
    t = table40()
    rows = np.array([BASE + 3, BASE + 39, BASE], np.uint32)
    bits = np.zeros(2, np.uint32)
    sentinel = 0xDEAD0000

    def from_rows(db, r, n, flags, out=True):
        h = C.c_void_p(sentinel)
        rc = L.gsim_rowset_from_rows(db, r, n, flags, C.byref(h) if out else None)
        return rc, h.value

    def from_bitmap(db, b, flags, out=True):
        h = C.c_void_p(sentinel)
        rc = L.gsim_rowset_from_bitmap(db, b, flags, C.byref(h) if out else None)
        return rc, h.value

    cases = {
        "NULL db": from_rows(None, u32(rows), 3, 0),
        "NULL rows with n > 0": from_rows(t._h, None, 3, 0),
        "unknown flag bits": from_rows(t._h, u32(rows), 3, 2),
        "unknown flag bits beside a known one": from_rows(t._h, u32(rows), 3, 1 | 4),
        "a row below the row base": from_rows(t._h, u32(np.array([BASE + 1, BASE - 1], np.uint32)), 2, 0),
        "a row past the table": from_rows(t._h, u32(np.array([BASE + 1, BASE + 40], np.uint32)), 2, 0),
        "a row without the base": from_rows(t._h, u32(np.array([5], np.uint32)), 1, 0),
        "bitmap: NULL db": from_bitmap(None, u32(bits), 0),
        "bitmap: NULL bits": from_bitmap(t._h, None, 0),
        "bitmap: unknown flag bits": from_bitmap(t._h, u32(bits), 8),
    }
    for what, (rc, h) in cases.items():  # (n >= 2^32: test_too_many_rows_is_invalid)
        assert rc == INVALID, what
        assert h is None, what + ": *out cleared"
    for what, rc in {"NULL out": from_rows(t._h, u32(rows), 3, 0, out=False)[0], "bitmap: NULL out": from_bitmap(t._h, u32(bits), 0, out=False)[0]}.items():
        assert rc == INVALID, what
    # every failure leaves a message
    for call in (lambda: from_rows(t._h, None, 3, 0), lambda: from_rows(t._h, u32(rows), 3, 2),
                 lambda: from_rows(t._h, u32(np.array([BASE + 40], np.uint32)), 1, 0), lambda: from_bitmap(t._h, None, 0)):
        assert call()[0] == INVALID and len(message()) > 0
    assert "outside" in (from_rows(t._h, u32(np.array([BASE + 40], np.uint32)), 1, 0), message())[1]
    t.close()


def test_too_many_rows_is_invalid():
    """n >= 2^32 is refused by its count alone: the rows are never read (the pointer holds one row)."""
    L = capi.load()
    t = table40()
    one = np.array([BASE], np.uint32)
    h = C.c_void_p(1)
    assert L.gsim_rowset_from_rows(t._h, u32(one), 1 << 32, 0, C.byref(h)) == INVALID
    assert h.value is None and "2^32" in message()
    t.close()


def test_a_table_not_on_a_gpu_is_a_state_error_after_the_argument_checks():
    L = capi.load()
    t = table40()
    rows = np.array([BASE + 3, BASE + 39, BASE, BASE + 3], np.uint32)  # valid: in range, a duplicate, any order
    for kw in (dict(rows=rows), dict(rows=rows, exclude=True), dict(rows=np.zeros(0, np.uint32)), dict(bitmap=np.array([5, 1], np.uint32)),
               dict(bitmap=np.array([5, 1], np.uint32), exclude=True)):
        with pytest.raises(capi.GsimError) as e:
            t.rowset(**kw)
        assert e.value.code == STATE, kw
        assert len(str(e.value)) > 0
    # ... and an argument error wins over it
    with pytest.raises(capi.GsimError) as e:
        t.rowset(rows=np.array([BASE + 40], np.uint32))
    assert e.value.code == INVALID
    h = C.c_void_p(7)
    assert L.gsim_rowset_from_rows(t._h, u32(rows), 4, 0, C.byref(h)) == STATE and h.value is None
    t.close()


def test_search_rows_argument_errors():
    L = capi.load()
    t = table40()
    q = np.zeros(32, np.uint32)
    hits = np.zeros(4, capi.HIT_DTYPE)
    counts = np.zeros(1, np.uint32)
    approx = np.zeros(1, np.uint64)
    # no row set can be made without a GPU; this is an object that belongs to no handle (every field zero)
    nobody = C.create_string_buffer(256)
    rs = C.cast(nobody, C.c_void_p)
    hp, cp, ap = hits.ctypes.data_as(C.c_void_p), u32(counts), approx.ctypes.data_as(C.POINTER(C.c_uint64))

    def call(db=t._h, rs=rs, queries=u32(q), hits=hp, counts=cp, metric=0):
        return L.gsim_db_search_rows(db, rs, queries, 1, 4, 0.0, metric, 1.0, 1.0, hits, counts, ap, None)

    for what, rc in {"NULL db": call(db=None), "NULL rs": call(rs=None), "NULL queries": call(queries=None), "NULL hits": call(hits=None),
                     "NULL counts": call(counts=None), "unknown metric": call(metric=7)}.items():
        assert rc == INVALID, what
        assert len(message()) > 0, what
    assert call() == INVALID and "another handle" in message()
    # gsim_rowset_count / _rows / _destroy
    n = C.c_uint64(5)
    assert L.gsim_rowset_count(None, C.byref(n)) == INVALID
    assert L.gsim_rowset_count(rs, None) == INVALID
    assert L.gsim_rowset_count(rs, C.byref(n)) == 0 and n.value == 0
    assert L.gsim_rowset_rows(None, u32(q)) == INVALID
    assert L.gsim_rowset_destroy(None) == 0
    t.close()
