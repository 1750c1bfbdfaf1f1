"""CPU checks of gsim_db_knn: the symbols exist and are exported, the stats struct and GSIM_KNN_MAX_K match the header, every
argument error of the contract is reported before any device state -- on a table that is not on a GPU -- with a message, one
argument changed at a time, `*out` is cleared on failure, a valid call on such a table is a state error (never a host computation),
and the numpy restatement of the rule (knn_rule.py) on a hand-worked 8-row table.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more -- at the narrowest width such a table is 16 GiB of host rows, more
than a test may build; the check is one comparison in gsim_db_knn, ahead of the state checks like the others."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi
from knn_rule import knn_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32
GARBAGE = 0xDEAD0


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in ("gsim_db_knn", "gsim_graph_get_knn_stats"):
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    assert capi.GsimKnnStats and capi.Table.knn
    from gpusimilarity_amd.fingerprintdb import FingerprintDB
    assert FingerprintDB.knn


def test_stats_struct_and_the_largest_k_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_knn_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    names = [n for _, n in fields]
    assert names == ["rows", "launches", "pairs", "inserts", "entries", "kernel_ms", "csr_ms", "d2h_ms", "wall_ms", "clock_mhz"]
    assert names == [n for n, _ in capi.GsimKnnStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimKnnStats._fields_]
    assert C.sizeof(capi.GsimKnnStats) == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_KNN_MAX_K\s+128u\b", text)
    assert capi.KNN_MAX_K == 128
    assert re.search(r"int gsim_db_knn\(gsim_db\* db, uint32_t k, float cutoff, int metric, float alpha, float beta,\s*"
                     r"uint64_t row_begin, uint64_t row_end, gsim_graph\*\* out\);", text)
    assert re.search(r"int gsim_graph_get_knn_stats\(const gsim_graph\* g, gsim_knn_stats\* out\);", text)


class Call:
    """gsim_db_knn on a table that is not on a GPU, one argument changed at a time; `out` holds garbage before every call."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.n = rows
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.out = C.c_void_p(GARBAGE)

    def __call__(self, db=True, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, row_begin=0, row_end=None, out=True):
        self.out = C.c_void_p(GARBAGE)
        return capi.load().gsim_db_knn(self.t._h if db else None, k, cutoff, metric, alpha, beta, row_begin,
                                       self.n if row_end is None else row_end, C.byref(self.out) if out else None)


def test_argument_errors_come_before_any_device_state():
    call = Call()
    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL db": dict(db=False), "NULL out": dict(out=False),
        "k 0": dict(k=0), "k above the largest": dict(k=capi.KNN_MAX_K + 1), "k huge": dict(k=0xFFFFFFFF),
        "cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff NaN": dict(cutoff=nan),
        "cutoff inf": dict(cutoff=inf),
        "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
        "negative alpha": dict(metric=TV, alpha=-0.5, beta=0.5), "negative beta": dict(metric=TV, alpha=0.5, beta=-0.5),
        "infinite alpha": dict(metric=TV, alpha=inf, beta=0.5), "infinite beta": dict(metric=TV, alpha=0.5, beta=inf),
        "NaN alpha": dict(metric=TV, alpha=nan, beta=0.5), "NaN beta": dict(metric=TV, alpha=0.5, beta=nan),
        "row_begin > row_end": dict(row_begin=7, row_end=6), "row_end past the count": dict(row_end=41),
        "both past the count": dict(row_begin=41, row_end=41),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
        if kw.get("out", True):
            assert call.out.value is None, ("*out is cleared on failure", what)
    call.t.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    assert wide() == INVALID and "4096" in message() and wide.out.value is None
    wide.t.close()
    widest = Call(bits=4096, rows=3)
    assert widest() == STATE
    widest.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    tiny = float(np.nextafter(F(0), F(1)))
    for kw in (dict(), dict(k=1), dict(k=capi.KNN_MAX_K), dict(cutoff=1.0), dict(cutoff=tiny), dict(row_begin=3, row_end=17),
               dict(row_begin=9, row_end=9), dict(row_begin=40, row_end=40), dict(metric=TV, alpha=0.5, beta=0.5),
               dict(metric=TV, alpha=0.3, beta=0.7), dict(metric=TV, alpha=1.0, beta=0.0), dict(metric=TV, alpha=0.0, beta=0.0),
               dict(metric=TAN, alpha=-1.0, beta=float("nan"))):
        assert call(**kw) == STATE, kw
        assert "GPU" in message(), kw
        assert call.out.value is None, kw
    assert call(cutoff=2.0) == INVALID, "an argument error wins over it"
    call.t.close()
    empty = Call(rows=0)
    assert empty() == STATE and empty(row_end=1) == INVALID
    empty.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.knn(3, 0.5)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        t.knn(3, 0.5, row_end=6)
    assert e.value.code == INVALID
    t.close()


def test_the_stats_accessor_rejects_a_null_graph():
    L = capi.load()
    st = capi.GsimKnnStats()
    assert L.gsim_graph_get_knn_stats(None, C.byref(st)) == INVALID and len(message()) > 0


def worked_table():
    """Eight rows, cutoff 0.3.  Row 6 is a duplicate of row 0 (1.0 against it, the same scores against everything else); row 3 is
    all-zero (NaN against everything, itself included); rows 1, 2 and 7 all score .8 against row 0 (and row 6): a tie group;
    score(1, 5) is exactly the cutoff; row 4 sees row 0 at .9 from ITS side only.  Unlisted pairs: 0.1."""
    nan = float("nan")
    m = np.full((8, 8), 0.1, np.float32)
    np.fill_diagonal(m, 1.0)
    for (i, j), v in {(0, 6): 1.0, (0, 1): .8, (0, 2): .8, (0, 7): .8, (6, 1): .8, (6, 2): .8, (6, 7): .8, (1, 2): .5, (1, 5): .3}.items():
        m[i, j] = m[j, i] = F(v)
    m[4, 0] = F(.9)  # the owner row is the query: no symmetry is assumed
    m[3, :] = nan
    m[:, 3] = nan
    return m


def lists(csr):
    indptr, indices, scores = csr
    return [(indices[int(a):int(b)].tolist(), scores[int(a):int(b)].tolist()) for a, b in zip(indptr[:-1], indptr[1:])]


def test_the_rule_on_a_hand_worked_table():
    m = worked_table()
    # k = 2.  Row 0: its duplicate first, then the tie group {1, 2, 7} at .8 cut to its lowest row.  Row 1: rows 0 and 6 tie at .8,
    # both fit.  Row 2 likewise.  Row 3 (all-zero): nothing, and it is in nobody's list.  Row 4: row 0 at .9, from its own side.
    # Row 5: row 1, exactly at the cutoff.  Row 6, the duplicate: row 0 at 1.0 (never itself), then row 1.  Row 7: rows 0 and 6.
    got = lists(knn_rule(m, 2, 0.3))
    assert [g[0] for g in got] == [[6, 1], [0, 6], [0, 6], [], [0], [1], [0, 1], [0, 6]]
    assert got[0][1] == [1.0, F(.8)] and got[4][1] == [F(.9)] and got[5][1] == [F(.3)]
    # k = 1: the duplicate alone; rows 1, 2 and 7 keep the lower of their two tied rows
    assert [g[0] for g in lists(knn_rule(m, 1, 0.3))] == [[6], [0], [0], [], [0], [1], [0], [0]]
    # k = 3: the tie group of row 0 is cut after its two lowest rows; row 1 adds row 2 (.5) and is then full
    got = lists(knn_rule(m, 3, 0.3))
    assert got[0][0] == [6, 1, 2] and got[6][0] == [0, 1, 2] and got[1][0] == [0, 6, 2]
    # k = 5: lists are shorter than k when fewer rows qualify; row 1 ends with row 5 at exactly the cutoff
    got = lists(knn_rule(m, 5, 0.3))
    assert [g[0] for g in got] == [[6, 1, 2, 7], [0, 6, 2, 5], [0, 6, 1], [], [0], [1], [0, 1, 2, 7], [0, 6]]
    assert got[1][1] == [F(.8), F(.8), F(.5), F(.3)]
    assert all(3 not in g[0] for g in got)
    # just above .3 the pair (1, 5) is gone from both sides
    above = float(np.nextafter(F(.3), F(1)))
    got = lists(knn_rule(m, 5, above))
    assert got[1][0] == [0, 6, 2] and got[5][0] == []
    # a range, and the row base on the indices and on nothing else
    indptr, indices, scores = knn_rule(m, 2, 0.3, row_begin=4, row_end=7, row_base=1000)
    assert indptr.tolist() == [0, 1, 2, 4] and indices.tolist() == [1000, 1001, 1000, 1001] and scores.tolist() == [F(.9), F(.3), 1.0, F(.8)]
    assert knn_rule(m, 2, 0.3, row_begin=5, row_end=5)[0].tolist() == [0]
