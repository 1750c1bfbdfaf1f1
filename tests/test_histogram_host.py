"""CPU checks of gsim_db_histogram / gsim_db_histogram_queries: the symbols exist and are exported, gsim_hist_stats and the two
constants match the header, every argument error of the contract is reported before any device state -- on tables that are not on
a GPU -- with a message, one argument changed at a time, an argument error wins over the state error, and a valid call on such a
table is a state error (never a host computation).
Not checked: GSIM_ERR_INVALID for 2^32 left rows or a table of 2^32 rows or more -- more host rows than a test may build; each is
one comparison ahead of the state checks, like the others."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32
U64P = C.POINTER(C.c_uint64)
FP = C.POINTER(C.c_float)


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in ("gsim_db_histogram", "gsim_db_histogram_queries"):
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    assert capi.GsimHistStats and capi.Table.histogram


def test_stats_struct_and_the_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_hist_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    names = [n for _, n in fields]
    assert names == ["left_rows", "rows_streamed", "rows_tiled", "stream_launches", "tile_launches", "pairs", "stream_ms", "tile_ms",
                     "reduce_ms", "d2h_ms", "wall_ms", "clock_mhz"]
    assert names == [n for n, _ in capi.GsimHistStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimHistStats._fields_]
    assert C.sizeof(capi.GsimHistStats) == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_HIST_MAX_EDGES\s+128u\b", text) and capi.HIST_MAX_EDGES == 128
    assert re.search(r"#define\s+GSIM_HIST_EXCLUDE_SELF\s+1u\b", text) and capi.HIST_EXCLUDE_SELF == 1
    text = re.sub(r"\s*/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int gsim_db_histogram_queries\(gsim_db\* db, const uint32_t\* queries, uint64_t nq,\s*"
                     r"const float\* edges, uint32_t nedges, int metric, float alpha, float beta,\s*"
                     r"uint64_t\* hist, uint64_t\* total,\s*gsim_hist_stats\* stats\);", text)
    assert re.search(r"int gsim_db_histogram\(gsim_db\* db, gsim_db\* left, uint64_t lrow_begin, uint64_t lrow_end,\s*"
                     r"const float\* edges, uint32_t nedges, int metric, float alpha, float beta, uint32_t flags,\s*"
                     r"uint64_t\* hist, uint64_t\* total, gsim_hist_stats\* stats\);", text)


EDGES = (0.25, 0.5, 0.75, 1.0)


class Call:
    """Either entry point on tables that are not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40, other_bits=None):
        W = bits // 32
        self.n, self.W = rows, W
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        ob = other_bits or bits
        self.other = capi.Table(ob).add_rows(np.ones((7, ob // 32), np.uint32))
        self.q = np.ones((3, W), np.uint32)

    def close(self):
        self.t.close()
        self.other.close()

    def outputs(self, nl, nb, hist, total):
        self.hist = np.zeros((max(nl, 1), nb), np.uint64)
        self.total = np.zeros(nb, np.uint64)
        return (self.hist.ctypes.data_as(U64P) if hist else None, self.total.ctypes.data_as(U64P) if total else None)

    def table(self, db=True, left="self", row_begin=0, row_end=None, edges=EDGES, nedges=None, metric=TAN, alpha=1.0, beta=1.0, flags=0,
              hist=True, total=True):
        lh = {"self": self.t, "other": self.other, None: None}[left]
        if row_end is None:
            row_end = lh.count() if lh else 0
        e = np.asarray(edges if edges is not None else [], F)
        n = len(e) if nedges is None else nedges
        hp, tp = self.outputs(max(row_end - row_begin, 0), len(e) + 1, hist, total)
        return capi.load().gsim_db_histogram(self.t._h if db else None, lh._h if lh else None, row_begin, row_end,
                                             e.ctypes.data_as(FP) if edges is not None else None, n, metric, alpha, beta, flags, hp, tp, None)

    def queries(self, db=True, q=True, nq=3, edges=EDGES, nedges=None, metric=TAN, alpha=1.0, beta=1.0, hist=True, total=True):
        e = np.asarray(edges if edges is not None else [], F)
        n = len(e) if nedges is None else nedges
        hp, tp = self.outputs(nq, len(e) + 1, hist, total)
        return capi.load().gsim_db_histogram_queries(self.t._h if db else None, self.q.ctypes.data_as(C.POINTER(C.c_uint32)) if q else None, nq,
                                                     e.ctypes.data_as(FP) if edges is not None else None, n, metric, alpha, beta, hp, tp, None)


inf, nan = float("inf"), float("nan")
COMMON = {
    "NULL db": dict(db=False),
    "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
    "negative alpha": dict(metric=TV, alpha=-0.5, beta=0.5), "negative beta": dict(metric=TV, alpha=0.5, beta=-0.5),
    "infinite alpha": dict(metric=TV, alpha=inf, beta=0.5), "NaN beta": dict(metric=TV, alpha=0.5, beta=nan),
    "NULL edges": dict(edges=None, nedges=4),
    "no edges": dict(edges=(), nedges=0), "nedges 0 with edges": dict(nedges=0),
    "129 edges": dict(edges=tuple((k + 1) / 130 for k in range(129))),
    "a descending pair": dict(edges=(0.25, 0.75, 0.5, 1.0)), "an equal pair": dict(edges=(0.25, 0.5, 0.5, 1.0)),
    "a NaN edge": dict(edges=(0.25, nan, 0.75)), "a NaN first edge": dict(edges=(nan, 0.5)), "an infinite edge": dict(edges=(0.25, 0.5, inf)),
    "edges[0] == 0": dict(edges=(0.0, 0.5)), "edges[0] < 0": dict(edges=(-0.25, 0.5)), "edges[0] == -0.0": dict(edges=(-0.0, 0.5)),
    "both outputs NULL": dict(hist=False, total=False),
}


def test_argument_errors_come_before_any_device_state():
    call = Call()
    for what, kw in COMMON.items():
        assert call.table(**kw) == INVALID, ("table", what)
        assert len(message()) > 0, what
        assert call.queries(**kw) == INVALID, ("queries", what)
        assert len(message()) > 0, what
    only_table = {
        "NULL left": dict(left=None),
        "unknown flag bits": dict(flags=2), "unknown flag bits beside the known one": dict(flags=0x80000001),
        "EXCLUDE_SELF with another handle": dict(left="other", flags=capi.HIST_EXCLUDE_SELF),
        "row_begin > row_end": dict(row_begin=7, row_end=6), "row_end past the count": dict(row_end=41),
        "row_end past the other handle's count": dict(left="other", row_end=8),
    }
    for what, kw in only_table.items():
        assert call.table(**kw) == INVALID, what
        assert len(message()) > 0, what
    assert call.queries(q=False) == INVALID and len(message()) > 0, "NULL queries with nq > 0"
    call.close()
    mixed = Call(bits=1024, other_bits=512)
    assert mixed.table(left="other") == INVALID and "fp_bits" in message()
    mixed.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    assert wide.table() == INVALID and "4096" in message()
    assert wide.queries() == INVALID and "4096" in message()
    wide.close()
    widest = Call(bits=4096, rows=3)
    assert widest.table() == STATE and widest.queries() == STATE
    widest.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    valid = (dict(), dict(edges=(0.5,)), dict(edges=tuple((k + 1) / 129 for k in range(128))), dict(edges=(0.5, 1.0, 1.5)),
             dict(edges=(float(np.nextafter(F(0), F(1))),)), dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=1.0, beta=0.0),
             dict(metric=TV, alpha=0.0, beta=0.0), dict(metric=TAN, alpha=-1.0, beta=nan), dict(hist=False), dict(total=False))
    for kw in valid:
        assert call.table(**kw) == STATE, kw
        assert "GPU" in message(), kw
        assert call.queries(**kw) == STATE, kw
        assert "GPU" in message(), kw
    for kw in (dict(flags=capi.HIST_EXCLUDE_SELF), dict(left="other"), dict(row_begin=3, row_end=17), dict(row_begin=9, row_end=9)):
        assert call.table(**kw) == STATE, kw
        assert "GPU" in message(), kw
    assert call.queries(nq=0, q=False) == STATE
    # an argument error wins over it
    assert call.table(edges=(0.5, 0.25)) == INVALID and call.queries(edges=(0.5, 0.25)) == INVALID
    assert call.table(hist=False, total=False) == INVALID and call.table(flags=4) == INVALID
    call.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.histogram(t, EDGES)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        t.histogram(np.ones((2, 32), np.uint32), EDGES)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.histogram(t, (0.5, 0.5))
    assert e.value.code == INVALID
    with pytest.raises(capi.GsimError) as e:
        t.histogram(t, EDGES, per_row=False, total=False)
    assert e.value.code == INVALID
    with pytest.raises(capi.GsimError) as e:
        t.histogram(np.ones((2, 32), np.uint32), EDGES, exclude_self=True)
    assert e.value.code == INVALID
    t.close()
