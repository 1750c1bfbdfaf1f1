"""CPU checks of gsim_db_snn / gsim_db_jarvis_patrick and of the host functions gsim_snn / gsim_jarvis_patrick: the symbols exist, the
stats struct, the flags and the prototypes match the header, every argument error of the two device calls is reported before any
device state -- on a table that is not on a GPU -- with a message, a valid call on such a table is a state error (never a host
computation), and the host functions against the Python restatement of the rule (jarvis_patrick_rule.py, the oracle of
tests/test_gpu_jarvis_patrick.py): a hand-worked graph of ten lists, 300 random list graphs, malformed graphs, and the mutual graph at
kmin = 0 against capi.components.  tests/cpp/snn_host_check.cpp, a stand-alone program, runs the same hand-worked graph with buffers
of exactly the promised sizes, built plainly and under the address and undefined-behaviour sanitizers.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more (16 GiB of host rows at the narrowest width)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jarvis_patrick_rule as R
from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
CLOSED, EITHER = capi.SNN_CLOSED, capi.SNN_EITHER
M = capi.SNN_MUTUAL_BIT
FLAGS = [dict(closed=c, either=e) for c in (False, True) for e in (False, True)]


def u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    names = ["gsim_db_snn", "gsim_graph_copy_shared", "gsim_graph_get_snn_stats", "gsim_db_jarvis_patrick", "gsim_snn", "gsim_jarvis_patrick"]
    for name in names:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.GsimSnnStats and capi.Table.snn and capi.Table.jarvis_patrick and capi.snn and capi.jarvis_patrick
    from gpusimilarity_amd.fingerprintdb import FingerprintDB
    assert FingerprintDB.jarvis_patrick


def test_stats_struct_flags_and_prototypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_snn_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+)(\[8\])?;", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    names = [n for _, n, _ in fields]
    assert names == ["rows", "k", "entries", "mutual_entries", "links", "unions", "cas_failed", "launches", "pairs", "inserts", "knn_ms",
                     "sort_ms", "link_ms", "label_ms", "d2h_ms", "wall_ms", "clock_mhz"]
    assert names == [n for n, _ in capi.GsimSnnStats._fields_]
    base = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [base[t] * 8 if arr else base[t] for t, _, arr in fields] == [t for _, t in capi.GsimSnnStats._fields_]
    assert C.sizeof(capi.GsimSnnStats) == 8 * (len(fields) + 7)
    assert re.search(r"#define\s+GSIM_SNN_CLOSED\s+1u\b", text) and CLOSED == 1
    assert re.search(r"#define\s+GSIM_SNN_EITHER\s+2u\b", text) and EITHER == 2
    assert re.search(r"#define\s+GSIM_SNN_MUTUAL_BIT\s+0x80000000u\b", text) and M == 0x80000000
    for proto in (
        r"int gsim_db_snn\(gsim_db\* db, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, gsim_graph\*\* out\);",
        r"int gsim_graph_copy_shared\(const gsim_graph\* g, uint32_t\* shared /\* nnz \*/\);",
        r"int gsim_graph_get_snn_stats\(const gsim_graph\* g, gsim_snn_stats\* out\);",
        r"int gsim_db_jarvis_patrick\(gsim_db\* db, uint32_t k, const uint32_t\* kmins, uint32_t nlevels, float cutoff, int metric, float alpha,",
        r"int gsim_snn\(const uint64_t\* indptr, const uint32_t\* indices, uint64_t nrows, uint32_t flags, uint32_t\* shared /\* nnz \*/\);",
        r"int gsim_jarvis_patrick\(const uint64_t\* indptr, const uint32_t\* indices, uint64_t nrows, const uint32_t\* kmins, uint32_t nlevels,",
    ):
        assert re.search(proto, text), proto


class Call:
    """The two device calls on a table that is not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.n = rows
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.cluster_of = np.zeros(8 * max(rows, 1), np.uint32)
        self.nclusters = np.full(8, 77, np.uint32)

    def jp(self, db=True, k=16, kmins=(8,), null_kmins=False, nlevels=None, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0,
           cluster_of=True, nclusters=True):
        km = np.ascontiguousarray(kmins, dtype=np.uint32)
        self.nclusters[:] = 77
        return capi.load().gsim_db_jarvis_patrick(
            self.t._h if db else None, k, None if null_kmins else u32(km), len(km) if nlevels is None else nlevels, cutoff, metric, alpha, beta,
            flags, u32(self.cluster_of) if cluster_of else None, u32(self.nclusters) if nclusters else None, None, None, None)

    def snn(self, db=True, k=16, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0, out=True):
        self.g = C.c_void_p(1234)
        return capi.load().gsim_db_snn(self.t._h if db else None, k, cutoff, metric, alpha, beta, flags, C.byref(self.g) if out else None)


inf, nan = float("inf"), float("nan")
LIST_ERRORS = {  # gsim_db_knn's checks of k, cutoff and metric: both calls
    "k 0": (dict(k=0), "k must be in"), "k 129": (dict(k=129), "k must be in"),
    "cutoff 0": (dict(cutoff=0.0), "cutoff"), "cutoff < 0": (dict(cutoff=-0.25), "cutoff"), "cutoff > 1": (dict(cutoff=1.0000001), "cutoff"),
    "cutoff NaN": (dict(cutoff=nan), "cutoff"), "cutoff inf": (dict(cutoff=inf), "cutoff"),
    "unknown metric": (dict(metric=7), "metric"), "negative metric": (dict(metric=-1), "metric"),
    "negative alpha": (dict(metric=TV, alpha=-0.5, beta=0.5), "alpha"), "infinite beta": (dict(metric=TV, alpha=0.5, beta=inf), "alpha"),
    "NaN weights": (dict(metric=TV, alpha=nan, beta=nan), "alpha"),
}


def test_argument_errors_of_jarvis_patrick_come_before_any_device_state():
    call = Call()
    cases = dict(LIST_ERRORS)
    cases.update({
        "NULL db": (dict(db=False), "NULL"), "flag 4": (dict(flags=4), "flags"), "all flag bits": (dict(flags=0xFFFFFFFF), "flags"),
        "NULL kmins": (dict(null_kmins=True), "NULL"), "NULL cluster_of": (dict(cluster_of=False), "NULL"),
        "NULL nclusters": (dict(nclusters=False), "NULL"),
        "no levels": (dict(nlevels=0), "levels"), "nine levels": (dict(kmins=[0, 1, 2, 3, 4, 5, 6, 7, 8]), "levels"),
        "kmin above k": (dict(kmins=[17]), "kmin"), "a later kmin above k": (dict(kmins=[3, 17]), "kmin"),
        "kmin above k + 2, closed": (dict(kmins=[19], flags=CLOSED), "kmin"), "k + 1 without closed": (dict(kmins=[17], flags=EITHER), "kmin"),
        "descending kmins": (dict(kmins=[8, 4]), "ascending"), "a repeated kmin": (dict(kmins=[3, 8, 8]), "ascending"),
    })
    for what, (kw, word) in cases.items():
        assert call.jp(**kw) == INVALID, what
        assert word in message(), (what, message())
    # the order: a bad k wins over bad flags, bad flags over a NULL output, that over the level count, that over the kmins
    assert call.jp(k=0, flags=4) == INVALID and "k must be in" in message()
    assert call.jp(flags=4, cluster_of=False) == INVALID and "flags" in message()
    assert call.jp(cluster_of=False, nlevels=0) == INVALID and "NULL" in message()
    assert call.jp(nlevels=9, kmins=[5, 4, 3, 2, 1, 0, 0, 0, 0]) == INVALID and "levels" in message()
    call.t.close()


def test_argument_errors_of_snn_come_before_any_device_state():
    call = Call()
    cases = dict(LIST_ERRORS)
    cases.update({"NULL db": (dict(db=False), "NULL"), "NULL out": (dict(out=False), "NULL"),
                  "the clustering's flag": (dict(flags=EITHER), "flags"), "flag 4": (dict(flags=4), "flags")})
    for what, (kw, word) in cases.items():
        assert call.snn(**kw) == INVALID, what
        assert word in message(), (what, message())
        assert not kw.get("out", True) or call.g.value is None, "*out is cleared on failure"
    call.t.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    assert wide.jp() == INVALID and "4096" in message()
    assert wide.snn() == INVALID and "4096" in message()
    wide.t.close()
    widest = Call(bits=4096, rows=3)
    assert widest.jp() == STATE and widest.snn() == STATE
    widest.t.close()


def test_an_empty_table_has_no_clusters():
    empty = Call(rows=0)
    assert empty.jp() == OK and empty.nclusters[0] == 0
    assert empty.jp(kmins=[0, 1, 2, 3, 4, 5, 6, 16]) == OK and not empty.nclusters.any()
    assert empty.jp(kmins=[17]) == INVALID, "an argument error still wins"
    empty.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    for kw in (dict(), dict(k=1, kmins=[0]), dict(k=128, kmins=[0, 128]), dict(kmins=[0, 18], flags=CLOSED), dict(flags=CLOSED | EITHER),
               dict(cutoff=1.0), dict(cutoff=1e-45), dict(metric=TV, alpha=0.9, beta=0.1), dict(metric=TAN, alpha=-1.0, beta=nan)):
        assert call.jp(**kw) == STATE, kw
        assert "GPU" in message(), kw
        assert not call.nclusters[:len(kw.get("kmins", [0]))].any()
    for kw in (dict(), dict(k=1), dict(k=128), dict(flags=CLOSED), dict(metric=TV, alpha=0.9, beta=0.1)):
        assert call.snn(**kw) == STATE and "GPU" in message(), kw
        assert call.g.value is None
    call.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.jarvis_patrick(4, 2, 0.5)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        t.jarvis_patrick(4, [2, 1], 0.5)
    assert e.value.code == INVALID
    with pytest.raises(capi.GsimError) as e:
        t.snn(4, 0.5)
    assert e.value.code == STATE
    t.close()


# ---- the host functions ----

WORKED = [[3, 1, 2], [0, 3, 2], [1, 0, 3], [2, 1, 0], [6, 5], [7, 4], [], [9, 8], [7, 9], [8, 0]]


def csr_of_lists(lists):
    indptr = np.zeros(len(lists) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(x) for x in lists])
    return indptr, np.array([j for x in lists for j in x], np.uint32)


def both(indptr, indices, kmins, what=None, **flags):
    """the rule and gsim_jarvis_patrick: they must agree; returns the levels as lists"""
    want = R.jarvis_patrick_rule(indptr, indices, kmins, **flags)
    got = capi.jarvis_patrick(indptr, indices, kmins, **flags)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            assert x.dtype == np.uint32 and x.tobytes() == y.tobytes(), (what, flags, kmins, x, y)
    return [[x.tolist() for x in g] for g in got]


def test_the_rule_and_the_host_functions_on_a_hand_worked_graph():
    """Rows 0 - 3 list each other (mutual, two rows shared); 4 and 5 list each other and share nothing; 6 has an empty list and is
    listed by 4 alone; 7 and 8 list each other and share 9; 7 lists 9 but 9 does not list 7, and they share 8; 8 and 9 list each other
    and share nothing; 9 lists 0."""
    indptr, indices = csr_of_lists(WORKED)
    open_, closed = capi.snn(indptr, indices), capi.snn(indptr, indices, closed=True)
    assert open_.tobytes() == R.snn_rule(indptr, indices).tobytes() and closed.tobytes() == R.snn_rule(indptr, indices, closed=True).tobytes()
    assert open_.tolist() == [M | 2] * 12 + [0, M, 0, M, 1, M | 1, M | 1, M, M, 0]
    assert closed.tolist() == [M | 4] * 12 + [1, M | 2, 1, M | 2, 2, M | 3, M | 3, M | 2, M | 2, 1]
    mutual_graph = [[0, 0, 0, 0, 1, 1, 2, 3, 3, 3], [0, 4, 6, 7], [4, 2, 1, 3]]
    pair_78 = [[0, 0, 0, 0, 1, 2, 3, 4, 4, 5], [0, 4, 5, 6, 7, 9], [4, 1, 1, 1, 2, 1]]
    clique = [[0, 0, 0, 0, 1, 2, 3, 4, 5, 6], [0, 4, 5, 6, 7, 8, 9], [4, 1, 1, 1, 1, 1, 1]]
    alone = [list(range(10)), list(range(10)), [1] * 10]
    one = [[0] * 10, [0], [10]]
    # the mutual pairs 4 - 5 and 8 - 9 share nothing: below kmin = 1
    assert both(indptr, indices, [0, 1, 2, 3]) == [mutual_graph, pair_78, clique, alone]
    # the one-sided pair 7 - 9 shares 8: only EITHER links it, at kmin 1; at 0 the entries 4 - 6, 5 - 7 and 9 - 0 join everything
    assert both(indptr, indices, [0, 1, 2, 3], either=True) == [one, [[0, 0, 0, 0, 1, 2, 3, 4, 4, 4], [0, 4, 5, 6, 7], [4, 1, 1, 1, 3]], clique, alone]
    # CLOSED: 4 - 5 counts 0 + 2, so it is a link at kmin 2, where the open rule has none
    assert both(indptr, indices, [0, 1, 2, 3], closed=True) == [mutual_graph, mutual_graph, mutual_graph, pair_78]
    assert both(indptr, indices, [0, 1, 2, 3], closed=True, either=True) == [one, one, mutual_graph, pair_78]
    assert both(indptr, indices, [2], closed=True)[0] != both(indptr, indices, [2])[0]
    assert R.stats_rule(indptr, indices, [0, 1, 2, 3]) == dict(entries=22, mutual_entries=18, links=[18, 14, 12, 0], unions=13)


def random_lists(rng):
    n = int(rng.integers(0, 61))
    lists = []
    for i in range(n):
        others = np.array([j for j in range(n) if j != i], np.int64)
        if rng.random() < 0.5 and n > 1:  # neighbours near the row: mutual pairs and shared rows are common
            others = others[np.argsort(np.abs(others - i) + rng.random(len(others)) * 4)][:14]
        m = min(int(rng.integers(0, 13)), len(others))
        lists.append(rng.permutation(rng.choice(others, m, replace=False)).tolist() if m else [])
    return lists


def test_the_host_functions_equal_the_rule_on_random_list_graphs():
    rng = np.random.default_rng(0x1A7B15)
    ladders = [[0], [1], [3], [0, 1, 2, 3, 4, 5, 6, 7], [1, 4], [2, 3, 9, 14], [0, 2, 4, 6, 13]]
    several = mutual = onesided = 0
    for g in range(300):
        lists = random_lists(rng)
        indptr, indices = csr_of_lists(lists)
        flags = FLAGS[g % 4]
        kmins = ladders[g % len(ladders)]
        levels = both(indptr, indices, kmins, what=g, **flags)
        for closed in (False, True):
            got, want = capi.snn(indptr, indices, closed=closed), R.snn_rule(indptr, indices, closed)
            assert got.tobytes() == want.tobytes(), (g, closed)
        mutual += int((want & M).any())
        onesided += int(len(want) > 0 and not (want & M).all())
        n = len(lists)
        several += int(any(1 < len(lv[1]) < n for lv in levels))
        for a, b in zip(levels, levels[1:]):  # refinement
            assert len(set(zip(a[0], b[0]))) == len(b[1])
    assert several >= 150 and mutual >= 250 and onesided >= 250, (several, mutual, onesided)


def raw(indptr, indices, nrows, kmins=(0,), flags=0):
    indptr = np.ascontiguousarray(indptr, np.uint64)
    indices = np.ascontiguousarray(indices, np.uint32)
    km = np.ascontiguousarray(kmins, np.uint32)
    out = np.zeros(max(nrows, 1) * len(km), np.uint32)
    nc = np.full(len(km), 99, np.uint32)
    rc = capi.load().gsim_jarvis_patrick(u64(indptr), u32(indices) if len(indices) else None, nrows, u32(km), len(km), flags, u32(out), None, None,
                                         u32(nc))
    shared = np.zeros(max(len(indices), 1), np.uint32)
    rc2 = capi.load().gsim_snn(u64(indptr), u32(indices) if len(indices) else None, nrows, flags & CLOSED, u32(shared))
    return rc, rc2, out[:nrows].tolist(), nc.tolist()


def test_malformed_graphs_are_invalid():
    for what, (indptr, indices, n) in {
        "indptr not starting at 0": ([1, 2, 2], [0, 1], 2), "indptr decreasing": ([0, 2, 1], [1, 0], 2),
        "a column outside the graph": ([0, 1, 2], [1, 2], 2), "NULL indices": ([0, 1, 2], [], 2),
        "a list that names its own row": ([0, 1, 2], [1, 1], 2), "a list that names a row twice": ([0, 2, 3, 3], [2, 2, 0], 3),
    }.items():
        rc, rc2, _, _ = raw(indptr, indices, n)
        assert rc == INVALID and len(message()) > 0, what
        assert rc2 == INVALID, what
    L = capi.load()
    zero, nc, km = np.zeros(1, np.uint64), np.zeros(8, np.uint32), np.array([0, 1], np.uint32)
    out = np.zeros(8, np.uint32)
    assert L.gsim_jarvis_patrick(None, None, 0, u32(km), 1, 0, None, None, None, u32(nc)) == INVALID
    assert L.gsim_jarvis_patrick(u64(zero), None, 0, None, 1, 0, None, None, None, u32(nc)) == INVALID
    assert L.gsim_jarvis_patrick(u64(zero), None, 0, u32(km), 1, 0, None, None, None, None) == INVALID
    two = np.zeros(3, np.uint64)
    assert L.gsim_jarvis_patrick(u64(two), None, 2, u32(km), 1, 0, None, None, None, u32(nc)) == INVALID, "NULL cluster_of with rows"
    assert L.gsim_jarvis_patrick(u64(two), None, 2, u32(km), 0, 0, u32(out), None, None, u32(nc)) == INVALID
    assert L.gsim_jarvis_patrick(u64(two), None, 2, u32(km), 9, 0, u32(out), None, None, u32(nc)) == INVALID
    assert L.gsim_jarvis_patrick(u64(two), None, 2, u32(km), 1, 4, u32(out), None, None, u32(nc)) == INVALID
    assert L.gsim_jarvis_patrick(u64(two), None, 2, u32(np.array([1, 1], np.uint32)), 2, 0, u32(out), None, None, u32(nc)) == INVALID
    assert L.gsim_snn(None, None, 0, 0, None) == INVALID and L.gsim_snn(u64(two), None, 2, 2, None) == INVALID
    # no rows, and rows without entries: legal; kmins are bounded only by being ascending
    assert raw([0], [], 0) == (OK, OK, [], [0])
    assert raw([0, 0, 0], [], 2, kmins=[0, 4000000000]) == (OK, OK, [0, 1], [2, 2])
    assert all(len(x) == 0 for x in capi.jarvis_patrick([0], [], 0)[0])
    with pytest.raises(capi.GsimError):
        capi.jarvis_patrick([0, 1, 2], [1, 0], [2, 1])


def test_kmin_0_mutual_on_a_symmetric_graph_is_its_components():
    rng = np.random.default_rng(0x5A11)
    for g in range(40):
        n = int(rng.integers(1, 120))
        U = np.triu(rng.random((n, n)) < float(rng.choice([0.5, 1.0, 2.0])) / n, 1)
        A = U | U.T
        lists = [rng.permutation(np.flatnonzero(A[i])).tolist() for i in range(n)]
        indptr, indices = csr_of_lists(lists)
        want = capi.components(indptr, indices)
        for flags in FLAGS:  # every pair is mutual, and every kmin-0 condition holds
            got = capi.jarvis_patrick(indptr, indices, 0, **flags)[0]
            for x, w in zip(got, want):
                assert x.tobytes() == w.tobytes(), (g, flags)


def test_the_stand_alone_checker_builds_plainly_and_under_the_sanitizers_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "snn_host_check.cpp")
    host = os.path.join(ROOT, "gpusimilarity_amd", "csrc", "capi_snn_host.cpp")
    deps = [src, host, os.path.join(ROOT, "include", "gpusim_hip.h")]
    common = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    for name, extra in (("snn_host_check", []),
                        ("snn_host_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exe = os.path.join(ROOT, "tests", "cpp", name)
        if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
            subprocess.check_call(common + extra + ["-o", exe, src, host])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], (name, r.stdout + r.stderr)
