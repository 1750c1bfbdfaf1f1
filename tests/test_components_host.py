"""CPU checks of gsim_db_components and gsim_components: the symbols exist, the stats struct and GSIM_COMPONENTS_MAX_LEVELS match the
header, the argument errors are reported before any device state -- on a table that is not on a GPU -- with a message, a valid call
on such a table is a state error (never a host computation), and gsim_components (host code) against the numpy restatement of the
rule (components_rule.py, the oracle of tests/test_gpu_components.py): a hand-worked 8-row table and 200 random graphs.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more -- at the narrowest width such a table is 16 GiB of host rows, more
than a test may build; the check is one comparison in gsim_db_components, ahead of the state checks like the others."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi
from components_rule import components_of_adjacency, components_rule, csr_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32


def u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    assert hasattr(L, "gsim_db_components") and hasattr(L, "gsim_components")
    assert "gsim_db_components" in capi.EXPORTS and "gsim_components" in capi.EXPORTS
    assert capi.GsimComponentsStats and capi.Table.components and capi.components


def test_stats_struct_and_the_level_limit_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_components_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    names = [n for _, n in fields]
    assert names == ["rows", "levels", "launches", "pairs", "kept", "unions", "cas_failed", "kernel_ms", "label_ms", "d2h_ms", "wall_ms",
                     "clock_mhz"]
    assert names == [n for n, _ in capi.GsimComponentsStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimComponentsStats._fields_]
    assert C.sizeof(capi.GsimComponentsStats) == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_COMPONENTS_MAX_LEVELS\s+8u\b", text)
    assert re.search(r"int gsim_db_components\(gsim_db\* db, const float\* cutoffs, uint32_t nlevels, int metric, float alpha, float beta,", text)
    assert re.search(r"int gsim_components\(const uint64_t\* indptr, const uint32_t\* indices, uint64_t nrows,", text)


class Call:
    """gsim_db_components on a table that is not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.n = rows
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.component_of = np.zeros(8 * max(rows, 1), np.uint32)
        self.ncomponents = np.full(8, 77, np.uint32)

    def __call__(self, db=True, cutoffs=(0.5,), null_cutoffs=False, nlevels=None, metric=TAN, alpha=1.0, beta=1.0, component_of=True,
                 ncomponents=True):
        cut = np.ascontiguousarray(cutoffs, dtype=np.float32)
        self.ncomponents[:] = 77
        return capi.load().gsim_db_components(
            self.t._h if db else None, None if null_cutoffs else cut.ctypes.data_as(C.POINTER(C.c_float)),
            len(cut) if nlevels is None else nlevels, metric, alpha, beta, u32(self.component_of) if component_of else None,
            u32(self.ncomponents) if ncomponents else None, None, None, None)


def test_argument_errors_come_before_any_device_state():
    call = Call()
    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL db": dict(db=False), "NULL cutoffs": dict(null_cutoffs=True), "NULL component_of": dict(component_of=False),
        "NULL ncomponents": dict(ncomponents=False),
        "no levels": dict(nlevels=0), "nine levels": dict(cutoffs=[.1, .2, .3, .4, .5, .6, .7, .8, .9]),
        "cutoff 0": dict(cutoffs=[0.0]), "cutoff < 0": dict(cutoffs=[-0.25]), "cutoff > 1": dict(cutoffs=[1.0000001]),
        "cutoff NaN": dict(cutoffs=[nan]), "cutoff inf": dict(cutoffs=[inf]),
        "a later cutoff 0": dict(cutoffs=[0.5, 0.0]), "a later cutoff > 1": dict(cutoffs=[0.5, 1.5]), "a later cutoff NaN": dict(cutoffs=[0.5, nan]),
        "descending cutoffs": dict(cutoffs=[0.7, 0.5]), "a repeated cutoff": dict(cutoffs=[0.3, 0.5, 0.5]),
        "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
        "asymmetric weights": dict(metric=TV, alpha=0.3, beta=0.7),
        "negative weights": dict(metric=TV, alpha=-0.5, beta=-0.5),
        "infinite weights": dict(metric=TV, alpha=inf, beta=inf), "NaN weights": dict(metric=TV, alpha=nan, beta=nan),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
    call.t.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    assert wide() == INVALID and "4096" in message()
    wide.t.close()
    widest = Call(bits=4096, rows=3)
    assert widest() == STATE
    widest.t.close()


def test_an_empty_table_has_no_components():
    empty = Call(rows=0)
    assert empty() == OK and empty.ncomponents[0] == 0
    assert empty(cutoffs=[.1, .2, .3, .4, .5, .6, .7, 1.0]) == OK and not empty.ncomponents.any()
    assert empty(cutoffs=[0.0]) == INVALID, "an argument error still wins"
    empty.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    for kw in (dict(), dict(cutoffs=[1.0]), dict(cutoffs=[1e-6]), dict(cutoffs=[.1, .2, .3, .4, .5, .6, .7, 1.0]),
               dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=0.0, beta=0.0), dict(metric=TAN, alpha=-1.0, beta=float("nan"))):
        assert call(**kw) == STATE, kw
        assert "GPU" in message(), kw
        assert not call.ncomponents[:len(kw.get("cutoffs", [0]))].any()
    assert call(cutoffs=[2.0]) == INVALID, "an argument error wins over it"
    call.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.components(0.5)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        t.components([0.5, 0.4])
    assert e.value.code == INVALID
    t.close()


def worked_table():
    """Eight rows.  0 - 1 - 2 is a chain whose ends are not adjacent (.6, .55, ends .1); row 3 is all-zero (NaN against everything);
    rows 4 and 6 are duplicates (1.0); rows 5 and 7 score exactly .5.  Unlisted pairs: 0.1."""
    nan = float("nan")
    m = np.full((8, 8), 0.1, np.float32)
    np.fill_diagonal(m, 1.0)
    for (i, j), v in {(0, 1): .6, (1, 2): .55, (4, 6): 1.0, (5, 7): .5}.items():
        m[i, j] = m[j, i] = F(v)
    m[3, :] = nan
    m[:, 3] = nan
    return m


def graph_at(m, cutoff):
    with np.errstate(invalid="ignore"):
        A = m >= F(cutoff)
    np.fill_diagonal(A, False)
    return A


def both(m, cutoff):
    """the rule and gsim_components on the graph at `cutoff`: they must agree; returns lists"""
    want = components_rule(m, cutoff)
    got = capi.components(*csr_of(graph_at(m, cutoff)))
    for g, w in zip(got, want[:3]):
        assert g.dtype == np.uint32 and np.array_equal(g, w), (cutoff, g, w)
    return [x.tolist() for x in got] + [want[3]]


def test_the_rule_and_the_host_function_on_a_hand_worked_table():
    m = worked_table()
    # .5: the chain is one component although its ends score .1; the zero row is alone; the duplicates; 5 - 7 at exactly the cutoff
    assert both(m, 0.5) == [[0, 0, 0, 1, 2, 3, 2, 3], [0, 3, 4, 5], [3, 1, 2, 2], 4]
    # one ulp above .5 the pair 5 - 7 is no edge
    above = float(np.nextafter(F(.5), F(1)))
    assert both(m, above) == [[0, 0, 0, 1, 2, 3, 2, 4], [0, 3, 4, 5, 7], [3, 1, 2, 1, 1], 3]
    # .6 is exactly the score of 0 - 1; 1 - 2 (.55) is gone
    assert both(m, 0.6) == [[0, 0, 1, 2, 3, 4, 3, 5], [0, 2, 3, 4, 5, 7], [2, 1, 1, 2, 1, 1], 2]
    assert both(m, float(np.nextafter(F(.6), F(1)))) == [[0, 1, 2, 3, 4, 5, 4, 6], [0, 1, 2, 3, 4, 5, 7], [1, 1, 1, 1, 2, 1, 1], 1]
    # 1.0: de-duplication
    assert both(m, 1.0) == [[0, 1, 2, 3, 4, 5, 4, 6], [0, 1, 2, 3, 4, 5, 7], [1, 1, 1, 1, 2, 1, 1], 1]
    # .1: everything but the zero row
    assert both(m, 0.1) == [[0, 0, 0, 1, 0, 0, 0, 0], [0, 3], [7, 1], 21]


def test_the_host_function_equals_the_rule_on_random_graphs():
    rng = np.random.default_rng(0xC0FFEE)
    several = 0
    for g in range(200):
        n = int(rng.integers(0, 301))
        density = float(rng.choice([0.0, 0.3 / max(n, 1), 1.0 / max(n, 1), 2.0 / max(n, 1), 0.05]))
        U = np.triu(rng.random((n, n)) < density, 1)
        A = U | U.T
        want = components_of_adjacency(A)
        got = capi.components(*csr_of(A))
        for x, w in zip(got, want):
            assert np.array_equal(x, w), (g, n, density)
        assert int(got[2].sum()) == n and len(got[1]) == len(got[2])
        several += int(1 < len(got[1]) < n)
    assert several >= 100, "most graphs have several components, some of them with several rows"


def raw(indptr, indices, nrows):
    indptr = np.ascontiguousarray(indptr, np.uint64)
    indices = np.ascontiguousarray(indices, np.uint32)
    out = np.zeros(max(nrows, 1), np.uint32)
    nc = C.c_uint64(99)
    rc = capi.load().gsim_components(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), u32(indices) if len(indices) else None, nrows, u32(out),
                                     None, None, C.byref(nc))
    return rc, out[:nrows].tolist(), nc.value


def test_malformed_graphs_are_invalid_and_odd_ones_harmless():
    for what, (indptr, indices, n) in {
        "indptr not starting at 0": ([1, 2, 2], [0, 1], 2), "indptr decreasing": ([0, 2, 1], [1, 0], 2),
        "a column outside the graph": ([0, 1, 2], [1, 2], 2), "NULL indices": ([0, 1, 2], [], 2),
    }.items():
        rc, _, _ = raw(indptr, indices, n)
        assert rc == INVALID and len(message()) > 0, what
    L = capi.load()
    nc = C.c_uint64(0)
    zero = np.zeros(1, np.uint64)
    assert L.gsim_components(None, None, 0, None, None, None, C.byref(nc)) == INVALID
    assert L.gsim_components(zero.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0, None, None, None, None) == INVALID
    assert L.gsim_components(zero.ctypes.data_as(C.POINTER(C.c_uint64)), None, 1, None, None, None, C.byref(nc)) == INVALID
    # no rows: legal
    assert raw([0], [], 0) == (OK, [], 0)
    got = capi.components([0], [])
    assert all(len(x) == 0 for x in got)
    # self edges and repeated edges change nothing; first_row and sizes may be left out
    assert raw([0, 3, 6, 7, 8], [0, 1, 1, 0, 0, 1, 2, 3], 4) == (OK, [0, 0, 1, 2], 3)
    # an edge listed under one of its rows only still joins them
    assert raw([0, 0, 0, 1], [0], 3) == (OK, [0, 1, 0], 2)
