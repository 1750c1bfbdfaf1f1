"""CPU checks of the group-query interface (gsim_db_search_group): the symbol exists, the stats struct and the hit match the
header, the argument errors are reported before any device state -- on a table that is not on a GPU -- with a message, and a
valid call on such a table is a state error, never a host computation.  Plus the bound the alpha / beta check rests on,
in f32, on the CPU.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more -- at the narrowest width such a table is 16 GiB of host rows, more
than a test may build; the check is one comparison in gsim_db_search_group, ahead of the state checks like the others."""
import ctypes as C
import os
import re

import numpy as np

from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY


def u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def message():
    return capi.load().gsim_last_error().decode()


def header():
    return open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()


def test_the_symbol_exists_and_is_exported():
    L = capi.load()
    assert hasattr(L, "gsim_db_search_group")
    assert "gsim_db_search_group" in capi.EXPORTS
    assert capi.GsimGroupStats and capi.Table.search_group
    assert (capi.GROUP_MAX, capi.GROUP_MIN, capi.GROUP_MEAN) == (0, 1, 2)


def test_stats_struct_and_constants_match_the_header():
    text = header()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_group_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == 6 and len(fields) == len(re.findall(r";", body)), "all uint64_t or double, as gsim_rowset_stats"
    assert [n for _, n in fields] == ["queries", "launches", "pairs", "scan_ms", "kernel_ms", "wall_ms"]
    assert [n for _, n in fields] == [n for n, _ in capi.GsimGroupStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimGroupStats._fields_]
    assert C.sizeof(capi.GsimGroupStats) == 8 * len(fields)
    for name, value in (("GSIM_GROUP_MAX", "0"), ("GSIM_GROUP_MIN", "1"), ("GSIM_GROUP_MEAN", "2"), ("GSIM_GROUP_MAX_QUERIES", "1024u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), text), name
    assert capi.GROUP_MAX_QUERIES == 1024


def test_the_hit_is_twelve_bytes_with_gsim_hits_layout():
    body = re.search(r"typedef struct \{([^}]*)\} gsim_group_hit;", header()).group(1)
    fields = re.findall(r"\b(uint32_t|float|uint16_t)\s+(\w+);", body)
    assert fields == [("uint32_t", "row"), ("float", "score"), ("uint16_t", "which"), ("uint16_t", "popc_db")]
    assert capi.GROUP_HIT_DTYPE.itemsize == 12 == capi.HIT_DTYPE.itemsize
    assert capi.GROUP_HIT_DTYPE.names == ("row", "score", "which", "popc_db")
    for name, other in zip(capi.GROUP_HIT_DTYPE.names, capi.HIT_DTYPE.names):
        assert capi.GROUP_HIT_DTYPE.fields[name][1] == capi.HIT_DTYPE.fields[other][1]
        assert capi.GROUP_HIT_DTYPE.fields[name][0] == capi.HIT_DTYPE.fields[other][0]


class Call:
    """gsim_db_search_group on a table that is not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.t = capi.Table(bits).add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.q = np.ones((3, W), np.uint32)
        self.hits = np.zeros(4, capi.GROUP_HIT_DTYPE)
        self.count = C.c_uint32(77)
        self.approx = C.c_uint64(0)

    def __call__(self, db=True, queries=True, nq=3, mode=0, k=4, cutoff=0.0, metric=TAN, alpha=1.0, beta=1.0, hits=True, count=True, approx=True):
        return capi.load().gsim_db_search_group(
            self.t._h if db else None, u32(self.q) if queries else None, nq, mode, k, cutoff, metric, alpha, beta,
            self.hits.ctypes.data_as(C.c_void_p) if hits else None, C.byref(self.count) if count else None,
            C.byref(self.approx) if approx else None, None)


def test_argument_errors_come_before_any_device_state():
    call = Call()
    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL db": dict(db=False), "NULL queries": dict(queries=False), "NULL hits": dict(hits=False), "NULL count": dict(count=False),
        "nq == 0": dict(nq=0), "nq above the limit": dict(nq=1025), "unknown mode": dict(mode=3), "negative mode": dict(mode=-1),
        "unknown metric": dict(metric=7),
        "Tversky alpha < 0": dict(metric=TV, alpha=-0.5, beta=2.0), "Tversky beta < 0": dict(metric=TV, alpha=2.0, beta=-0.25),
        "Tversky alpha + beta < 1": dict(metric=TV, alpha=0.3, beta=0.6), "Tversky 0 / 0": dict(metric=TV, alpha=0.0, beta=0.0),
        "Tversky alpha inf": dict(metric=TV, alpha=inf, beta=1.0), "Tversky beta nan": dict(metric=TV, alpha=1.0, beta=nan),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
    assert call(nq=1025) == INVALID and "1024" in message()
    # Tanimoto ignores alpha and beta, as gsim_db_search does
    assert call(metric=TAN, alpha=-1.0, beta=nan) == STATE
    call.t.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    assert wide() == INVALID and "4096" in message()
    wide.t.close()
    widest = Call(bits=4096, rows=3)
    assert widest() == STATE
    widest.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    for kw in (dict(), dict(mode=1), dict(mode=2, k=0), dict(nq=1), dict(metric=TV, alpha=0.3, beta=0.7), dict(metric=TV, alpha=1.0, beta=0.0),
               dict(metric=TV, alpha=0.0, beta=1.0), dict(approx=False), dict(cutoff=0.5)):
        assert call(**kw) == STATE, kw
        assert "GPU" in message(), kw
    # ... and an argument error wins over it
    assert call(mode=5) == INVALID
    call.t.close()
    import pytest
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.search_group(np.ones((2, 32), np.uint32), 3, capi.GROUP_MEAN)
    assert e.value.code == STATE and len(str(e.value)) > 0
    t.close()


def test_accepted_weights_bound_every_f32_score_by_one():
    """The check accepts alpha, beta >= 0 with alpha + beta >= 1; the bound score <= 1 needs alpha, beta >= 0 alone: with the scan's
    arithmetic (one f32 rounding per operation) den = fl(fl(fl(alpha (a - c)) + fl(beta (b - c))) + c) >= c.  Every (a, b, c) of a
    256-bit row, for weights at the edge of what is accepted (and tiny, huge and subnormal ones): no counterexample."""
    f = np.float32
    weights = [(1.0, 0.0), (0.0, 1.0), (0.3, 0.7), (0.5, 0.5), (1e-45, 1.0), (1.0, 1e-45), (3e38, 3e38), (1.0, 3e38), (0.99999994, 5.9604645e-08),
               (16777216.0, 0.0), (0.0, 16777217.0)]
    a, b, c = np.meshgrid(np.arange(0, 257, 7), np.arange(0, 257, 5), np.arange(0, 257), indexing="ij")
    ok = (c <= a) & (c <= b)
    a, b, c = a[ok].astype(np.int64), b[ok].astype(np.int64), c[ok].astype(np.int64)
    # the widest rows' extremes as well
    a = np.concatenate([a, [4096, 4096, 4095, 1]]); b = np.concatenate([b, [4096, 1, 4096, 4096]]); c = np.concatenate([c, [4096, 1, 4095, 1]])
    for alpha, beta in weights:
        assert float(f(alpha)) + float(f(beta)) >= 1.0
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            t1 = (f(alpha) * (a - c).astype(f)).astype(f)
            t2 = (f(beta) * (b - c).astype(f)).astype(f)
            den = ((t1 + t2).astype(f) + c.astype(f)).astype(f)
            s = (c.astype(f) / den).astype(f)
        assert np.all(den >= c.astype(f)), (alpha, beta)
        assert np.all(np.isnan(s) | ((s >= 0) & (s <= 1))), (alpha, beta)
        assert np.all(np.isnan(s) <= (c == 0)), "NaN only as 0 / 0"
