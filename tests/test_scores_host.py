"""CPU checks of gsim_db_scores / gsim_db_scores_queries / gsim_db_scores_device: the symbols exist and are exported,
gsim_scores_stats matches the header field by field, every argument error of the contract is reported before any device state -- on
tables that are not on a GPU -- with a message and with the output buffer untouched, one argument changed at a time, an argument
error wins over the state error, and a valid call on such a table is a state error (never a host computation).
2^32 rows or more on one side: checked through the queries entry, which refuses nq = 2^32 by its count alone (the rows are never
read).  Not reachable on a host table: 2^32 left rows of a handle or 2^32 table rows -- the range check against the handle's count
comes first, and no test may build that many rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
FP = C.POINTER(C.c_float)
U32P = C.POINTER(C.c_uint32)
FILL = 0x7FC12345  # a NaN's bit pattern: no score ever equals it
NAMES = ("gsim_db_scores", "gsim_db_scores_queries", "gsim_db_scores_device")


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    assert capi.GsimScoresStats and capi.Table.scores


def test_stats_struct_and_the_prototypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_scores_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"\b(uint64_t|double)\s+([\w\s,]+);", body):
        fields += [(typ, n.strip()) for n in names.split(",")]
    assert len(re.findall(r";", body)) == 9, "uint64_t and double declarations only, as the other stats structs"
    names = [n for _, n in fields]
    assert names == ["left_rows", "right_rows", "launches", "slabs", "pairs", "prepare_ms", "kernel_ms", "d2h_ms", "wall_ms", "clock_mhz"]
    assert names == [n for n, _ in capi.GsimScoresStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimScoresStats._fields_]
    assert C.sizeof(capi.GsimScoresStats) == 8 * len(fields)
    text = re.sub(r"\s*/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int gsim_db_scores\(gsim_db\* db, gsim_db\* left, uint64_t lrow_begin, uint64_t lrow_end,\s*"
                     r"uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha, float beta,\s*"
                     r"float\* out, uint64_t ld, gsim_scores_stats\* stats\);", text)
    assert re.search(r"int gsim_db_scores_queries\(gsim_db\* db, const uint32_t\* queries, uint64_t nq,\s*"
                     r"uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha, float beta,\s*"
                     r"float\* out, uint64_t ld, gsim_scores_stats\* stats\);", text)
    assert re.search(r"int gsim_db_scores_device\(gsim_db\* db, gsim_db\* left, uint64_t lrow_begin, uint64_t lrow_end,\s*"
                     r"uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha, float beta,\s*"
                     r"void\* d_out, uint64_t ld, gsim_scores_stats\* stats\);", text)


class Call:
    """The three entry points on tables that are not on a GPU, one argument changed at a time.  The output buffer (host memory for
    all three: nothing may touch it before the state check) is prefilled with FILL."""

    def __init__(self, bits=1024, rows=40, other_bits=None):
        W = bits // 32
        self.W = W
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        ob = other_bits or bits
        self.other = capi.Table(ob).add_rows(np.ones((7, ob // 32), np.uint32))
        self.q = np.ones((3, W), np.uint32)
        self.buf = None

    def close(self):
        self.t.close()
        self.other.close()

    def output(self, out):
        self.buf = np.full(64 * 64, FILL, np.uint32)
        return self.buf.ctypes.data_as(FP) if out else None

    def untouched(self):
        return bool((self.buf == FILL).all())

    def table(self, entry="gsim_db_scores", db=True, left="self", row_begin=0, row_end=None, col_begin=0, col_end=None, metric=TAN, alpha=1.0,
              beta=1.0, out=True, ld=None):
        lh = {"self": self.t, "other": self.other, None: None}[left]
        if row_end is None:
            row_end = lh.count() if lh else 0
        if col_end is None:
            col_end = self.t.count()
        if ld is None:
            ld = max(col_end - col_begin, 0)
        o = self.output(out)
        if entry == "gsim_db_scores_device":
            o = C.cast(o, C.c_void_p)
        return getattr(capi.load(), entry)(self.t._h if db else None, lh._h if lh else None, row_begin, row_end, col_begin, col_end, metric,
                                           alpha, beta, o, ld, None)

    def device(self, **kw):
        return self.table(entry="gsim_db_scores_device", **kw)

    def queries(self, db=True, q=True, nq=3, col_begin=0, col_end=None, metric=TAN, alpha=1.0, beta=1.0, out=True, ld=None):
        if col_end is None:
            col_end = self.t.count()
        if ld is None:
            ld = max(col_end - col_begin, 0)
        return capi.load().gsim_db_scores_queries(self.t._h if db else None, self.q.ctypes.data_as(U32P) if q else None, nq, col_begin, col_end,
                                                  metric, alpha, beta, self.output(out), ld, None)


inf, nan = float("inf"), float("nan")
COMMON = {
    "NULL db": dict(db=False),
    "NULL out": dict(out=False),
    "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
    "negative alpha": dict(metric=TV, alpha=-0.5, beta=0.5), "negative beta": dict(metric=TV, alpha=0.5, beta=-0.5),
    "infinite alpha": dict(metric=TV, alpha=inf, beta=0.5), "NaN beta": dict(metric=TV, alpha=0.5, beta=nan),
    "ld < nr": dict(ld=39), "ld < nr of a range": dict(col_begin=10, col_end=30, ld=19), "ld 0": dict(ld=0),
    "col_begin > col_end": dict(col_begin=7, col_end=6, ld=40), "col_end past the count": dict(col_end=41, ld=41),
}


def test_argument_errors_come_before_any_device_state():
    call = Call()
    for what, kw in COMMON.items():
        for entry in (call.table, call.device, call.queries):
            assert entry(**kw) == INVALID, (entry.__name__, what)
            assert len(message()) > 0, what
            assert call.untouched(), what
    only_handles = {
        "NULL left": dict(left=None),
        "row_begin > row_end": dict(row_begin=7, row_end=6), "row_end past the count": dict(row_end=41),
        "row_end past the other handle's count": dict(left="other", row_end=8),
    }
    for what, kw in only_handles.items():
        for entry in (call.table, call.device):
            assert entry(**kw) == INVALID, (entry.__name__, what)
            assert len(message()) > 0, what
            assert call.untouched(), what
    assert call.queries(q=False) == INVALID and len(message()) > 0 and call.untouched(), "NULL queries with nq > 0"
    assert call.queries(nq=1 << 32) == INVALID and "2^32" in message() and call.untouched(), "2^32 left rows"
    assert call.queries(nq=(1 << 32) - 1) == STATE, "one fewer is a valid count"
    call.close()
    mixed = Call(bits=1024, other_bits=512)
    for entry in (mixed.table, mixed.device):
        assert entry(left="other") == INVALID and "fp_bits" in message() and mixed.untouched()
    mixed.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    for entry in (wide.table, wide.device, wide.queries):
        assert entry() == INVALID and "4096" in message() and wide.untouched()
    wide.close()
    widest = Call(bits=4096, rows=3)
    for entry in (widest.table, widest.device, widest.queries):
        assert entry() == STATE
    widest.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    valid = (dict(), dict(ld=40), dict(ld=1000), dict(col_begin=5, col_end=17), dict(col_begin=5, col_end=17, ld=64), dict(col_begin=9, col_end=9),
             dict(col_begin=9, col_end=9, out=False), dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=0.3, beta=0.7),
             dict(metric=TV, alpha=0.0, beta=0.0), dict(metric=TAN, alpha=-1.0, beta=nan))
    for kw in valid:
        for entry in (call.table, call.device, call.queries):
            assert entry(**kw) == STATE, (entry.__name__, kw)
            assert "GPU" in message(), kw
            assert call.untouched(), kw
    for kw in (dict(left="other"), dict(row_begin=3, row_end=17), dict(row_begin=9, row_end=9), dict(row_begin=9, row_end=9, out=False)):
        for entry in (call.table, call.device):
            assert entry(**kw) == STATE, (entry.__name__, kw)
            assert "GPU" in message() and call.untouched(), kw
    assert call.queries(nq=0, q=False) == STATE and call.queries(nq=0, q=False, out=False) == STATE
    # an argument error wins over it
    assert call.table(ld=39) == INVALID and call.device(metric=9) == INVALID and call.queries(col_end=41, ld=41) == INVALID
    call.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.scores(t)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        t.scores(np.ones((2, 32), np.uint32))
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.scores(t, metric=TV, alpha=-1.0)
    assert e.value.code == INVALID
    with pytest.raises(capi.GsimError) as e:
        t.scores(t, col_end=6)
    assert e.value.code == INVALID
    with pytest.raises(capi.GsimError) as e:
        t.scores(np.ones((2, 32), np.uint32), out_ptr=4096)  # an array as the left side together with out_ptr
    assert e.value.code == INVALID
    t.close()
