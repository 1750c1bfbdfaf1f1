"""CPU checks of gsim_db_knn_join / gsim_db_knn_queries: the symbols exist and are exported, the stats struct and
GSIM_KNN_EXCLUDE_SELF match the header, every argument error of the contract is reported before any device state -- on tables that
are not on a GPU -- with a message, one argument changed at a time, `*out` is cleared on failure, a valid call on such tables is a
state error (never a host computation), the stats accessors refuse each other's graphs and NULL, the numpy restatement of the rule
(knn_join_rule.py) on a hand-worked rectangular table, and the launch plan (tests/cpp/knn_join_plan_check.cpp, built and run).
Not checked: GSIM_ERR_INVALID for nl >= 2^32 or a table of 2^32 rows or more -- at the narrowest width such a table is 16 GiB of host
rows, more than a test may build; each check is one comparison ahead of the state checks like the others.  The accessors' refusal of
a REAL graph of another kind needs a graph, hence a GPU: tests/test_gpu_knn_join.py has it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusimilarity_amd import capi
from knn_join_rule import knn_join_rule
from knn_rule import knn_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32
GARBAGE = 0xDEAD0
NEW = ["gsim_db_knn_join", "gsim_db_knn_queries", "gsim_graph_get_knn_join_stats"]
FIELDS = ["left_rows", "table_rows", "segments", "fold_launches", "merge_launches", "pairs", "inserts", "partial_entries", "entries",
          "kernel_ms", "merge_ms", "csr_ms", "d2h_ms", "wall_ms", "clock_mhz"]


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    assert capi.GsimKnnJoinStats and capi.Table.knn_join
    from gpusimilarity_amd.fingerprintdb import FingerprintDB
    assert FingerprintDB.knn_join


def test_stats_struct_and_the_flag_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_knn_join_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    names = [n for _, n in fields]
    assert names == FIELDS
    assert names == [n for n, _ in capi.GsimKnnJoinStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimKnnJoinStats._fields_]
    assert C.sizeof(capi.GsimKnnJoinStats) == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_KNN_EXCLUDE_SELF\s+1u\b", text) and capi.KNN_EXCLUDE_SELF == 1
    assert re.search(r"int gsim_db_knn_join\(gsim_db\* db, gsim_db\* left, uint64_t lrow_begin, uint64_t lrow_end, uint32_t k, float cutoff,\s*"
                     r"int metric, float alpha, float beta, uint32_t flags, gsim_graph\*\* out\);", text)
    assert re.search(r"int gsim_db_knn_queries\(gsim_db\* db, const uint32_t\* queries, uint64_t nq, uint32_t k, float cutoff,\s*"
                     r"int metric, float alpha, float beta, gsim_graph\*\* out\);", text)
    assert re.search(r"int gsim_graph_get_knn_join_stats\(const gsim_graph\* g, gsim_knn_join_stats\* out\);", text)


def host_table(bits, rows):
    W = bits // 32
    t = capi.Table(bits)
    if rows:
        t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
    return t


class Call:
    """gsim_db_knn_join on tables that are not on a GPU, one argument changed at a time; `out` holds garbage before every call."""

    def __init__(self, bits=1024, rows=40, lrows=30, lbits=None):
        self.nl = lrows
        self.t = host_table(bits, rows)
        self.left = host_table(lbits or bits, lrows)
        self.out = C.c_void_p(GARBAGE)

    def __call__(self, db=True, left="other", lrow_begin=0, lrow_end=None, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0,
                 out=True):
        self.out = C.c_void_p(GARBAGE)
        lh = {"other": self.left._h, "same": self.t._h, None: None}[left]
        if lrow_end is None:
            lrow_end = self.t.count() if left == "same" else self.nl
        return capi.load().gsim_db_knn_join(self.t._h if db else None, lh, lrow_begin, lrow_end, k, cutoff, metric, alpha, beta, flags,
                                            C.byref(self.out) if out else None)

    def close(self):
        self.t.close()
        self.left.close()


class QCall:
    """gsim_db_knn_queries likewise."""

    def __init__(self, bits=1024, rows=40, nq=7):
        self.t = host_table(bits, rows)
        self.q = np.ones((nq, bits // 32), np.uint32)
        self.out = C.c_void_p(GARBAGE)

    def __call__(self, db=True, queries=True, nq=None, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, out=True):
        self.out = C.c_void_p(GARBAGE)
        qp = self.q.ctypes.data_as(C.POINTER(C.c_uint32)) if queries else None
        return capi.load().gsim_db_knn_queries(self.t._h if db else None, qp, len(self.q) if nq is None else nq, k, cutoff, metric, alpha,
                                               beta, C.byref(self.out) if out else None)


inf, nan = float("inf"), float("nan")
SHARED = {
    "NULL db": dict(db=False), "NULL out": dict(out=False),
    "k 0": dict(k=0), "k above the largest": dict(k=capi.KNN_MAX_K + 1), "k huge": dict(k=0xFFFFFFFF),
    "cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff NaN": dict(cutoff=nan),
    "cutoff inf": dict(cutoff=inf),
    "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
    "negative alpha": dict(metric=TV, alpha=-0.5, beta=0.5), "negative beta": dict(metric=TV, alpha=0.5, beta=-0.5),
    "infinite alpha": dict(metric=TV, alpha=inf, beta=0.5), "infinite beta": dict(metric=TV, alpha=0.5, beta=inf),
    "NaN alpha": dict(metric=TV, alpha=nan, beta=0.5), "NaN beta": dict(metric=TV, alpha=0.5, beta=nan),
}


def check_invalid(call, cases):
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
        if kw.get("out", True):
            assert call.out.value is None, ("*out is cleared on failure", what)


def test_argument_errors_of_the_handle_call_come_before_any_device_state():
    call = Call()
    cases = dict(SHARED)
    cases.update({
        "NULL left": dict(left=None),
        "unknown flag bits": dict(flags=2), "unknown flag bits beside the known one": dict(left="same", flags=3), "all flag bits": dict(flags=0xFFFFFFFF),
        "the self flag with left != db": dict(flags=capi.KNN_EXCLUDE_SELF),
        "lrow_begin > lrow_end": dict(lrow_begin=7, lrow_end=6), "lrow_end past the left count": dict(lrow_end=31),
        "both past the left count": dict(lrow_begin=31, lrow_end=31),
        "lrow_end past the count, left == db": dict(left="same", lrow_end=41),
        "a range of the table's size on a shorter left table": dict(lrow_end=40),
    })
    check_invalid(call, cases)
    call.close()
    other = Call(bits=1024, lbits=512)
    assert other() == INVALID and "fp_bits" in message() and other.out.value is None
    other.close()


def test_argument_errors_of_the_queries_call_come_before_any_device_state():
    call = QCall()
    cases = dict(SHARED)
    cases["NULL queries with nq > 0"] = dict(queries=False)
    check_invalid(call, cases)
    assert call(queries=False, nq=0) == STATE, "NULL queries are legal with nq == 0"
    call.t.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3, lrows=3)
    assert wide() == INVALID and "4096" in message() and wide.out.value is None
    wide.close()
    widest = Call(bits=4096, rows=3, lrows=3)
    assert widest() == STATE
    widest.close()
    q = QCall(bits=4128, rows=3)
    assert q() == INVALID and "4096" in message() and q.out.value is None
    q.t.close()


def test_a_valid_call_on_tables_not_on_a_gpu_is_a_state_error():
    call = Call()
    tiny = float(np.nextafter(F(0), F(1)))
    for kw in (dict(), dict(k=1), dict(k=capi.KNN_MAX_K), dict(cutoff=1.0), dict(cutoff=tiny), dict(lrow_begin=3, lrow_end=17),
               dict(lrow_begin=9, lrow_end=9), dict(lrow_begin=30, lrow_end=30), dict(metric=TV, alpha=0.5, beta=0.5),
               dict(metric=TV, alpha=0.3, beta=0.7), dict(metric=TV, alpha=1.0, beta=0.0), dict(metric=TV, alpha=0.0, beta=0.0),
               dict(metric=TAN, alpha=-1.0, beta=nan), dict(left="same"), dict(left="same", flags=capi.KNN_EXCLUDE_SELF),
               dict(left="same", lrow_begin=5, lrow_end=40, flags=capi.KNN_EXCLUDE_SELF)):
        assert call(**kw) == STATE, kw
        assert "GPU" in message(), kw
        assert call.out.value is None, kw
    assert call(cutoff=2.0) == INVALID, "an argument error wins over it"
    call.close()
    q = QCall()
    for kw in (dict(), dict(k=capi.KNN_MAX_K), dict(nq=1), dict(nq=0), dict(metric=TV, alpha=0.3, beta=0.7)):
        assert q(**kw) == STATE and "GPU" in message() and q.out.value is None, kw
    assert q(k=0) == INVALID
    with pytest.raises(capi.GsimError) as e:
        q.t.knn_join(q.q, 3, 0.5)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        q.t.knn_join(q.t, 3, 0.5, row_end=41)
    assert e.value.code == INVALID
    with pytest.raises(capi.GsimError) as e:
        q.t.knn_join(q.t, 3, 0.5, exclude_self=True)
    assert e.value.code == STATE
    with pytest.raises(ValueError):
        q.t.knn_join(q.q, 3, 0.5, exclude_self=True)
    q.t.close()


def test_the_stats_accessors_reject_null():
    L = capi.load()
    st = capi.GsimKnnJoinStats()
    assert L.gsim_graph_get_knn_join_stats(None, C.byref(st)) == INVALID and len(message()) > 0
    assert L.gsim_graph_get_knn_stats(None, C.byref(capi.GsimKnnStats())) == INVALID
    assert L.gsim_graph_get_join_stats(None, C.byref(capi.GsimJoinStats())) == INVALID


def worked_table():
    """Five left rows against eight table rows, cutoff 0.3.  Left row 0 scores 1.0 against table rows 2 and 6 (duplicates of it)
    and .8 against rows 1, 4 and 7: a tie group.  Left row 1 is all-zero (NaN against everything).  Table row 3 is all-zero (NaN
    against everybody).  Left row 2 scores exactly the cutoff against row 5 and nothing else above it.  Left row 3 has nothing at
    the cutoff.  Left row 4 ties at .5 against rows 0, 1, 2, 4, 5, 6, 7.  Unlisted pairs: 0.1."""
    m = np.full((5, 8), 0.1, np.float32)
    m[0, [2, 6]] = 1.0
    m[0, [1, 4, 7]] = F(.8)
    m[2, 5] = F(.3)
    m[4, :] = F(.5)
    m[1, :] = nan
    m[:, 3] = nan
    return m


def lists(csr):
    indptr, indices, scores = csr
    return [(indices[int(a):int(b)].tolist(), scores[int(a):int(b)].tolist()) for a, b in zip(indptr[:-1], indptr[1:])]


def test_the_rule_on_a_hand_worked_table():
    m = worked_table()
    # k = 3: row 0 takes both duplicates, then the tie group {1, 4, 7} cut to its lowest row; row 4's tie group is cut after 0, 1, 2
    got = lists(knn_join_rule(m, 3, 0.3))
    assert [g[0] for g in got] == [[2, 6, 1], [], [5], [], [0, 1, 2]]
    assert got[0][1] == [1.0, 1.0, F(.8)] and got[2][1] == [F(.3)]
    # k = 1: the lower duplicate alone
    assert [g[0] for g in lists(knn_join_rule(m, 1, 0.3))] == [[2], [], [5], [], [0]]
    # k = 8: shorter than k when fewer rows qualify; the all-zero table row 3 is in nobody's list
    got = lists(knn_join_rule(m, 8, 0.3))
    assert [g[0] for g in got] == [[2, 6, 1, 4, 7], [], [5], [], [0, 1, 2, 4, 5, 6, 7]]
    assert all(3 not in g[0] for g in got)
    # just above .3 the pair (2, 5) is gone
    assert lists(knn_join_rule(m, 8, float(np.nextafter(F(.3), F(1)))))[2][0] == []
    # a range of left rows, and the TABLE's row base on the indices and on nothing else
    indptr, indices, scores = knn_join_rule(m, 2, 0.3, lrow_begin=2, lrow_end=5, row_base=1000)
    assert indptr.tolist() == [0, 1, 1, 3] and indices.tolist() == [1005, 1000, 1001] and scores.tolist() == [F(.3), F(.5), F(.5)]
    assert knn_join_rule(m, 2, 0.3, lrow_begin=3, lrow_end=3)[0].tolist() == [0]


def test_with_the_self_flag_the_rule_is_gsim_db_knns():
    """On a square matrix with the pair (i, i) left out the rule is knn_rule; without the flag a non-zero row lists itself or a
    lower-numbered duplicate first, at 1.0."""
    rng = np.random.default_rng(0x4A01)
    n = 40
    S = rng.choice(np.array([.125, .25, .5, .625, .75], F), (n, n))
    np.fill_diagonal(S, 1.0)
    S[7, 3] = S[3, 7] = 1.0  # rows 3 and 7 are duplicates
    S[11, :] = nan
    S[:, 11] = nan
    for k in (1, 4, 40):
        for lo, hi in ((0, n), (5, 23)):
            a = knn_join_rule(S, k, 0.25, lrow_begin=lo, lrow_end=hi, row_base=9, exclude_self=True)
            b = knn_rule(S, k, 0.25, row_begin=lo, row_end=hi, row_base=9)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, lo, hi)
    first = lists(knn_join_rule(S, 1, 0.25))
    assert [g[0] for g in first] == [[i] if i not in (7, 11) else ([3] if i == 7 else []) for i in range(n)]
    assert all(g[1] == [1.0] for i, g in enumerate(first) if i != 11)


def test_the_launch_plan_checker_builds_plainly_and_passes():
    """tests/cpp/knn_join_plan_check.cpp: plan_knn_join over a grid of (nl, N, WP, CUs, knobs) -- every (owner tile, column) folded
    exactly once, segment cuts at multiples of 256 and ascending, S by the rule and the clamp, the partial lists within the stated
    bound, a segment's launches in ascending column order."""
    src = os.path.join(ROOT, "tests", "cpp", "knn_join_plan_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "knn_join_plan_check")
    libdir = os.path.join(ROOT, "gpusimilarity_amd")
    csrc = os.path.join(libdir, "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    deps = [src, os.path.join(csrc, "capi_pairs.h"), os.path.join(csrc, "gsim_device.h"), os.path.join(libdir, "libgsim_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-o", exe, src, "-L" + libdir, "-lgsim_hip", "-Wl,-rpath," + libdir,
                               "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout + r.stderr
