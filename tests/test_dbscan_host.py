"""CPU checks of gsim_db_dbscan and its host companion gsim_dbscan: the symbols exist, the struct matches the header, the argument
errors are reported before any device state -- on a table that is not on a GPU -- with a message and each with its code, a valid call
on such a table is a state error (never a host computation), and gsim_dbscan against the Python restatement of the rule
(dbscan_rule.py): a hand-worked 12-row graph with cores, a border row whose two best core neighbours tie across clusters, one whose
better score sits on the larger row, and noise; 300 random symmetric graphs whose scores are drawn from 4 or 5 values (ties dominate)
for min_pts in {1, 2, 3, 5}; with min_pts == 1 the result equals capi.components.  Malformed graphs and NaN scores are rejected.
tests/cpp/dbscan_host_check.cpp, a stand-alone program over gsim_dbscan with buffers of exactly the promised sizes, is built plainly and
run.  Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more (as tests/test_components_host.py says of gsim_db_components)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusimilarity_amd import capi
from dbscan_rule import NOISE, census, dbscan_rule
from test_mst_host import both_ways, csr, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32
NEW = ["gsim_db_dbscan", "gsim_dbscan"]


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.Table.dbscan and capi.dbscan
    from gpusimilarity_amd.fingerprintdb import FingerprintDB
    assert FingerprintDB.dbscan


def test_the_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    assert re.search(r"#define\s+GSIM_DBSCAN_NOISE\s+0xFFFFFFFFu\b", text) and capi.DBSCAN_NOISE == 0xFFFFFFFF == NOISE
    fields = struct_fields(text, "gsim_dbscan_stats")
    scalar = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [n for _, n in fields] == ["rows", "launches_count", "launches_link", "pairs", "kept", "cores", "borders", "noise", "clusters",
                                      "unions", "cas_failed", "count_ms", "link_ms", "label_ms", "d2h_ms", "wall_ms", "clock_mhz"]
    assert [(n, scalar[t]) for t, n in fields] == list(capi.GsimDbscanStats._fields_)
    assert C.sizeof(capi.GsimDbscanStats) == 8 * 17
    assert re.search(r"int gsim_db_dbscan\(gsim_db\* db, float cutoff, uint32_t min_pts, int metric, float alpha, float beta,\s+uint32_t\* label_of", text)
    assert re.search(r"int gsim_dbscan\(const uint64_t\* indptr, const uint32_t\* indices, const float\* scores, uint64_t nrows, uint32_t min_pts,", text)


class Call:
    """gsim_db_dbscan on a table that is not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.out = [np.full(max(rows, 1), 0x5A5A5A5A, np.uint32) for _ in range(5)]
        self.ncl = C.c_uint32(77)

    def __call__(self, db=True, cutoff=0.5, min_pts=3, metric=TAN, alpha=1.0, beta=1.0, label_of=True, nclusters=True, optional=True):
        self.ncl.value = 77
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        opt = [u32(a) if optional else None for a in self.out[1:]]
        return capi.load().gsim_db_dbscan(self.t._h if db else None, cutoff, min_pts, metric, alpha, beta, u32(self.out[0]) if label_of else None,
                                          C.byref(self.ncl) if nclusters else None, *opt, None)


def test_argument_errors_come_before_any_device_state():
    call = Call()
    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL db": dict(db=False), "NULL label_of": dict(label_of=False), "NULL nclusters": dict(nclusters=False),
        "cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff NaN": dict(cutoff=nan),
        "cutoff inf": dict(cutoff=inf), "min_pts 0": dict(min_pts=0),
        "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
        "asymmetric weights": dict(metric=TV, alpha=0.3, beta=0.7), "negative weights": dict(metric=TV, alpha=-0.5, beta=-0.5),
        "infinite weights": dict(metric=TV, alpha=inf, beta=inf), "NaN weights": dict(metric=TV, alpha=nan, beta=nan),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
        assert kw.get("nclusters", True) is False or call.ncl.value == 0, what
        assert all((a == 0x5A5A5A5A).all() for a in call.out), (what, "no output is touched")
    assert "min_pts" in (call(min_pts=0), message())[1]
    call.t.close()
    wide = Call(bits=4128, rows=3)
    assert wide() == INVALID and "4096" in message()
    wide.t.close()
    widest = Call(bits=4096, rows=3)
    assert widest() == STATE
    widest.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    tiny = float(np.nextafter(F(0), F(1)))
    for kw in (dict(), dict(cutoff=1.0), dict(cutoff=tiny), dict(min_pts=1), dict(min_pts=0xFFFFFFFF), dict(optional=False),
               dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=0.0, beta=0.0), dict(metric=TAN, alpha=-1.0, beta=float("nan"))):
        assert call(**kw) == STATE, kw
        assert "GPU" in message() and call.ncl.value == 0, kw
    assert call(cutoff=2.0) == INVALID and call(min_pts=0) == INVALID, "an argument error wins over it"
    call.t.close()
    one = Call(rows=1)
    assert one() == STATE, "one row still needs a table on a GPU"
    one.t.close()
    empty = Call(rows=0)
    assert empty() == OK and empty.ncl.value == 0 and empty(optional=False) == OK
    assert empty(cutoff=0.0) == INVALID and empty(min_pts=0) == INVALID, "an argument error still wins"
    label_of, degree, anchor, first_row, sizes, st = empty.t.dbscan(0.5, 3)
    assert all(len(x) == 0 and x.dtype == np.uint32 for x in (label_of, degree, anchor, first_row, sizes))
    assert st["rows"] == st["clusters"] == st["launches_count"] == st["launches_link"] == 0
    assert empty.t.dbscan(0.5, 3, degree=False, anchor=False, first_row=False, sizes=False)[1:5] == (None, None, None, None)
    empty.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.dbscan(0.5, 3)
    assert e.value.code == STATE and len(str(e.value)) > 0
    t.close()


def matrix_of(n, a, b, s):
    """the score matrix dbscan_rule reads: an edge's score in the upper triangle, 0 elsewhere (0 is never >= the cutoff used)"""
    S = np.zeros((n, n), F)
    S[a, b] = s
    return S


CUT = 0.01  # below every score drawn: the edges are the listed pairs


def test_a_hand_worked_graph():
    """Twelve rows, min_pts = 4 (a core has at least three neighbours).  0 - 3 and 5 - 8 are cliques at .75 and .5: two clusters of
    cores.  Row 4 lies next to 3 and to 5 at .25 each: a border row whose best core neighbours tie across the clusters, and the smaller
    row, 3, wins.  Row 9 lies next to 0 at .125 and to 8 at .25: the better score wins although it sits on the larger row.  Rows 10 and
    11 only know each other, at .875: no core neighbour, noise, however good the score."""
    pairs = ([(a, b, .75) for a in range(4) for b in range(a + 1, 4)] + [(a, b, .5) for a in range(5, 9) for b in range(a + 1, 9)] +
             [(3, 4, .25), (4, 5, .25), (8, 9, .25), (0, 9, .125), (10, 11, .875)])
    N = NOISE
    indptr, indices, scores = csr(12, both_ways(pairs))
    label_of, anchor, first_row, sizes = capi.dbscan(indptr, indices, scores, 4)
    assert label_of.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, N, N]
    assert anchor.tolist() == [0, 1, 2, 3, 3, 5, 6, 7, 8, 8, N, N]
    assert first_row.tolist() == [0, 5] and sizes.tolist() == [5, 5]
    a, b, s = (np.array(x) for x in zip(*pairs))
    want = dbscan_rule(matrix_of(12, a.astype(int), b.astype(int), s.astype(F)), CUT, 4)
    assert [x.tolist() for x in (want[0], want[2], want[3], want[4])] == [label_of.tolist(), anchor.tolist(), [0, 5], [5, 5]]
    assert census(want) == (8, 2, 2, 2)
    # the listing's order plays no part, and a self edge is not a neighbour: row 9 with one stays a border row (degree 2)
    rng = np.random.default_rng(5)
    listed = both_ways(pairs) + [(9, 9, 1.0)]
    again = capi.dbscan(*csr(12, [listed[k] for k in rng.permutation(len(listed))]), 4)
    assert all(np.array_equal(x, y) for x, y in zip(again, (label_of, anchor, first_row, sizes)))
    # min_pts = 3: rows 4 and 9 have two neighbours and are cores now: they bridge the cliques into one cluster
    label_of, anchor, first_row, sizes = capi.dbscan(indptr, indices, scores, 3)
    assert label_of.tolist() == [0] * 10 + [N, N] and anchor.tolist() == list(range(10)) + [N, N] and sizes.tolist() == [10]
    # min_pts = 2: any row with a neighbour is a core, so there are no border rows; 1: every row is
    for mp in (2, 1):
        label_of, anchor, first_row, sizes = capi.dbscan(indptr, indices, scores, mp)
        assert label_of.tolist() == [0] * 10 + [1, 1] and anchor.tolist() == list(range(12)) and first_row.tolist() == [0, 10]
    # min_pts = 6: nobody has five neighbours
    label_of, anchor, first_row, sizes = capi.dbscan(indptr, indices, scores, 6)
    assert (label_of == N).all() and (anchor == N).all() and len(first_row) == len(sizes) == 0


def random_graph(rng):
    n = int(rng.integers(0, 121))
    values = rng.choice(np.array([.125, .25, .5, .625, .75, 1.0], F), int(rng.integers(4, 6)), replace=False)
    density = float(rng.choice([0.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0]) / max(n, 1))
    a, b = np.nonzero(np.triu(rng.random((n, n)) < density, 1))
    return n, a, b, rng.choice(values, len(a)).astype(F)


def test_the_host_function_equals_the_rule_on_random_graphs_full_of_ties():
    rng = np.random.default_rng(0xDB5CA)
    tied = cross = with_borders = with_noise = several = 0
    for g in range(300):
        n, a, b, s = random_graph(rng)
        S = matrix_of(n, a, b, s)
        listed = both_ways(zip(a.tolist(), b.tolist(), s.tolist()))
        indptr, indices, scores = csr(n, [listed[k] for k in rng.permutation(len(listed))])
        for mp in (1, 2, 3, 5):
            want = dbscan_rule(S, CUT, mp)
            got = capi.dbscan(indptr, indices, scores, mp)
            for x, y, what in zip(got, (want[0], want[2], want[3], want[4]), ("label_of", "anchor", "first_row", "sizes")):
                assert x.dtype == np.uint32 and x.tobytes() == y.tobytes(), (g, n, mp, what)
            cores, borders, noise, clusters = census(want)
            with_borders += borders > 0
            with_noise += noise > 0
            several += clusters > 1
            # how often the rule's tie-break decided: a border row whose best score is held by several cores, in several clusters
            label_of, _, anchor, _, _, _ = want
            sym = S + S.T
            for x in np.flatnonzero((anchor != np.arange(n)) & (anchor != NOISE)):
                near = np.flatnonzero((sym[x] > 0) & (anchor == np.arange(n)))
                top = near[sym[x, near] == sym[x, near].max()]
                tied += len(top) > 1
                cross += len(set(label_of[top].tolist())) > 1
            if mp == 1:
                comp = capi.components(indptr, indices)
                assert all(np.array_equal(p, q) for p, q in zip((got[0], got[2], got[3]), comp)), (g, n)
                assert np.array_equal(got[1], np.arange(n))
    assert tied >= 200 and cross >= 20 and with_borders >= 150 and with_noise >= 300 and several >= 200, (tied, cross, with_borders, with_noise, several)


def test_malformed_input_is_invalid():
    L = capi.load()
    nc = C.c_uint64(5)
    out = [np.zeros(8, np.uint32) for _ in range(4)]
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def raw(indptr, indices, scores, n, min_pts=2, null_label=False):
        indptr, indices, scores = np.ascontiguousarray(indptr, np.uint64), np.ascontiguousarray(indices, np.uint32), np.ascontiguousarray(scores, F)
        return L.gsim_dbscan(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), u32(indices) if len(indices) else None,
                             scores.ctypes.data_as(C.POINTER(C.c_float)) if len(scores) else None, n, min_pts,
                             None if null_label else u32(out[0]), u32(out[1]), u32(out[2]), u32(out[3]), C.byref(nc))

    for what, args in {
        "indptr not starting at 0": ([1, 2, 2], [0, 1], [.5, .5], 2), "indptr decreasing": ([0, 2, 1], [1, 0], [.5, .5], 2),
        "a column outside the graph": ([0, 1, 2], [1, 2], [.5, .5], 2), "NULL indices": ([0, 1, 2], [], [.5, .5], 2),
        "NULL scores": ([0, 1, 2], [1, 0], [], 2), "a NaN score": ([0, 1, 2], [1, 0], [.5, float("nan")], 2),
        "min_pts 0": ([0, 1, 2], [1, 0], [.5, .5], 2, 0), "NULL label_of": ([0, 1, 2], [1, 0], [.5, .5], 2, 2, True),
    }.items():
        assert raw(*args) == INVALID and len(message()) > 0 and nc.value == 0, what
    assert L.gsim_dbscan(None, None, None, 0, 2, None, None, None, None, C.byref(nc)) == INVALID
    assert raw([0, 1, 2], [1, 0], [.5, .5], 2) == OK and nc.value == 1 and out[0][:2].tolist() == [0, 0]
    assert raw([0], [], [], 0) == OK and nc.value == 0, "no rows: legal"
    assert raw([0], [], [], 0, 2, True) == OK, "no rows need no label buffer"
    assert all(len(x) == 0 for x in capi.dbscan([0], [], [], 3))
    # the optional outputs
    ip = np.array([0, 1, 2], np.uint64)
    assert L.gsim_dbscan(ip.ctypes.data_as(C.POINTER(C.c_uint64)), u32(np.array([1, 0], np.uint32)),
                         np.array([.5, .5], F).ctypes.data_as(C.POINTER(C.c_float)), 2, 2, u32(out[0]), None, None, None, C.byref(nc)) == OK
    with pytest.raises(capi.GsimError):
        capi.dbscan([0, 1, 2], [1, 0], [.5], 2)


def test_the_stand_alone_checker_builds_plainly_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "dbscan_host_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "dbscan_host_check")
    libdir = os.path.join(ROOT, "gpusimilarity_amd")
    deps = [src, os.path.join(ROOT, "include", "gpusim_hip.h"), os.path.join(libdir, "libgsim_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + libdir, "-lgsim_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout + r.stderr
