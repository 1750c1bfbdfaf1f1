"""CPU checks of gsim_db_mst and its host companions gsim_mst, gsim_mst_linkage and gsim_mst_cut: the symbols exist, the structs match
the header, the argument errors are reported before any device state -- on a table that is not on a GPU -- with a message, a valid call
on such a table is a state error (never a host computation), and the three host functions against the Python restatement of the rule
(mst_rule.py): a hand-worked 8-row graph, 200 random scored graphs whose scores are drawn from at most 6 values (ties dominate), cuts
against gsim_components of the thresholded graph, the dendrogram's sizes, ids and -- against scipy -- its merge heights.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more (as tests/test_components_host.py says of gsim_db_components)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi
from mst_rule import EDGE, kruskal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32
NEW = ["gsim_db_mst", "gsim_mst", "gsim_mst_linkage", "gsim_mst_cut"]


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.Table.mst and capi.mst and capi.mst_linkage and capi.mst_cut


def struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(.*\S)\s*$", decl, flags=re.S)
        if m:
            fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return fields


def test_structs_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    assert struct_fields(text, "gsim_mst_edge") == [("uint32_t", "a"), ("uint32_t", "b"), ("float", "score")]
    assert capi.MST_EDGE_DTYPE.names == ("a", "b", "score") and capi.MST_EDGE_DTYPE.itemsize == 12 and capi.MST_EDGE_DTYPE == EDGE
    assert struct_fields(text, "gsim_mst_merge") == [("uint32_t", "left"), ("uint32_t", "right"), ("float", "score"), ("uint32_t", "size")]
    assert capi.MST_MERGE_DTYPE.names == ("left", "right", "score", "size") and capi.MST_MERGE_DTYPE.itemsize == 16
    assert re.search(r"#define\s+GSIM_MST_MAX_ROUNDS\s+33u\b", text) and capi.MST_MAX_ROUNDS == 33
    fields = struct_fields(text, "gsim_mst_stats")
    scalar = {"uint64_t": C.c_uint64, "double": C.c_double}
    want = [(n, scalar[t]) if "[" not in n else (n.split("[")[0], scalar[t] * 33) for t, n in fields]
    assert [n for n, _ in want] == ["rows", "rounds", "scans", "launches", "pairs", "owner_rows", "edges", "kernel_ms", "round_ms", "sort_ms",
                                    "d2h_ms", "wall_ms", "clock_mhz", "scan_owners", "scan_kernel_ms"]
    assert all(n.endswith("[GSIM_MST_MAX_ROUNDS]") for _, n in fields[-2:])
    assert [(n, C.sizeof(t)) for n, t in want] == [(n, C.sizeof(t)) for n, t in capi.GsimMstStats._fields_]
    assert C.sizeof(capi.GsimMstStats) == 8 * (13 + 2 * 33)
    assert re.search(r"int gsim_db_mst\(gsim_db\* db, float cutoff, int metric, float alpha, float beta,\s+gsim_mst_edge\* edges", text)


class Call:
    """gsim_db_mst on a table that is not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.edges = np.zeros(max(rows, 2), capi.MST_EDGE_DTYPE)
        self.nedges = C.c_uint64(77)

    def __call__(self, db=True, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, edges=True, nedges=True):
        self.nedges.value = 77
        return capi.load().gsim_db_mst(self.t._h if db else None, cutoff, metric, alpha, beta, self.edges.ctypes.data if edges else None,
                                       C.byref(self.nedges) if nedges else None, None)


def test_argument_errors_come_before_any_device_state():
    call = Call()
    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL db": dict(db=False), "NULL edges": dict(edges=False), "NULL nedges": dict(nedges=False),
        "cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff NaN": dict(cutoff=nan),
        "cutoff inf": dict(cutoff=inf),
        "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
        "asymmetric weights": dict(metric=TV, alpha=0.3, beta=0.7), "negative weights": dict(metric=TV, alpha=-0.5, beta=-0.5),
        "infinite weights": dict(metric=TV, alpha=inf, beta=inf), "NaN weights": dict(metric=TV, alpha=nan, beta=nan),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
        assert kw.get("nedges", True) is False or call.nedges.value == 0, what
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
    for kw in (dict(), dict(cutoff=1.0), dict(cutoff=tiny), dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=0.0, beta=0.0),
               dict(metric=TAN, alpha=-1.0, beta=float("nan"))):
        assert call(**kw) == STATE, kw
        assert "GPU" in message() and call.nedges.value == 0, kw
    assert call(cutoff=2.0) == INVALID, "an argument error wins over it"
    call.t.close()
    one = Call(rows=1)
    assert one() == STATE and one(edges=False) == STATE, "one row needs no edge buffer, but still a table on a GPU"
    one.t.close()
    empty = Call(rows=0)
    assert empty() == OK and empty.nedges.value == 0 and empty(edges=False) == OK
    assert empty(cutoff=0.0) == INVALID, "an argument error still wins"
    edges, st = empty.t.mst(0.5)
    assert len(edges) == 0 and edges.dtype == capi.MST_EDGE_DTYPE and st["rows"] == st["edges"] == st["scans"] == 0
    empty.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.mst(0.5)
    assert e.value.code == STATE and len(str(e.value)) > 0
    t.close()


def csr(n, listed):
    """CSR of the (row, column, score) entries as listed: nothing is added, merged or mirrored"""
    listed = sorted(listed, key=lambda e: e[0])
    indptr = np.zeros(n + 1, np.uint64)
    for r, _, _ in listed:
        indptr[r + 1] += 1
    return np.cumsum(indptr).astype(np.uint64), np.array([c for _, c, _ in listed], np.uint32), np.array([s for _, _, s in listed], F)


def both_ways(pairs):
    pairs = list(pairs)
    return [(a, b, s) for a, b, s in pairs] + [(b, a, s) for a, b, s in pairs]


def as_list(edges):
    return [(int(e["a"]), int(e["b"]), float(e["score"])) for e in edges]


def test_a_hand_worked_graph():
    """Eight rows.  0 - 1 - 2 is a chain with equal scores (.5, .5); the pair (0, 1) is listed twice under row 0; row 3 is isolated;
    4, 5, 6 are a cycle of three edges tied at .75, whose E-last edge (5, 6) must be the one left out; 7 hangs on 2 at .25; the chain's
    ends (0, 2) score .125, below both of its links: never taken."""
    pairs = [(0, 1, .5), (1, 2, .5), (0, 2, .125), (4, 5, .75), (4, 6, .75), (5, 6, .75), (2, 7, .25)]
    listed = both_ways(pairs) + [(0, 1, .5), (6, 6, 1.0)]  # a repeated pair and a self edge: harmless
    want = [(4, 5, .75), (4, 6, .75), (0, 1, .5), (1, 2, .5), (2, 7, .25)]
    got = capi.mst(*csr(8, listed))
    assert got.dtype == capi.MST_EDGE_DTYPE and as_list(got) == want
    # an edge listed under one of its rows only still counts; the order of the listing plays no part
    assert as_list(capi.mst(*csr(8, pairs[::-1]))) == want
    # the dendrogram: ids 8 .. 12 in edge order; left holds the smaller smallest row
    merges = capi.mst_linkage(got, 8)
    assert [tuple(m) for m in merges.tolist()] == [(4, 5, .75, 2), (8, 6, .75, 3), (0, 1, .5, 2), (10, 2, .5, 3), (11, 7, .25, 4)]
    # cuts: exactly at a score, and one ulp above it
    comp, first, sizes = capi.mst_cut(got, 8, 0.5)
    assert comp.tolist() == [0, 0, 0, 1, 2, 2, 2, 3] and first.tolist() == [0, 3, 4, 7] and sizes.tolist() == [3, 1, 3, 1]
    comp, first, sizes = capi.mst_cut(got, 8, float(np.nextafter(F(.5), F(1))))
    assert comp.tolist() == [0, 1, 2, 3, 4, 4, 4, 5] and sizes.tolist() == [1, 1, 1, 1, 3, 1]
    comp, first, sizes = capi.mst_cut(got, 8, 0.0)
    assert comp.tolist() == [0, 0, 0, 1, 2, 2, 2, 0] and first.tolist() == [0, 3, 4] and sizes.tolist() == [4, 1, 3]
    assert capi.mst_cut(got[::-1], 8, 0.5)[0].tolist() == [0, 0, 0, 1, 2, 2, 2, 3], "a cut takes the edges in any order"


def random_graph(rng):
    n = int(rng.integers(0, 121))
    values = rng.choice(np.array([.125, .25, .5, .625, .75, 1.0], F), int(rng.integers(1, 7)), replace=False)
    density = float(rng.choice([0.0, 0.5 / max(n, 1), 1.5 / max(n, 1), 3.0 / max(n, 1), 0.1, 0.6]))
    a, b = np.nonzero(np.triu(rng.random((n, n)) < density, 1))
    return n, a.astype(np.uint32), b.astype(np.uint32), rng.choice(values, len(a)).astype(F)


def test_the_host_functions_equal_the_rule_on_random_graphs_full_of_ties():
    rng = np.random.default_rng(0x3157)
    tied = several = cycles = 0
    for g in range(200):
        n, a, b, s = random_graph(rng)
        want = kruskal(a, b, s, n)
        listed = both_ways(zip(a.tolist(), b.tolist(), s.tolist()))
        indptr, indices, scores = csr(n, [listed[k] for k in rng.permutation(len(listed))])
        got = capi.mst(indptr, indices, scores)
        assert got.tobytes() == want.tobytes(), (g, n)
        _, counts = np.unique(got["score"], return_counts=True)
        tied += int(counts[counts > 1].sum()) * 2 >= len(got) > 0
        cycles += len(a) > len(got)
        # cuts at every distinct score (and between, and beyond): gsim_components of the thresholded graph
        for t in sorted(set(s.tolist()) | {0.0, 0.3, 2.0}):
            keep = s >= F(t)
            kl = both_ways(zip(a[keep].tolist(), b[keep].tolist(), s[keep].tolist()))
            ci, cx, _ = csr(n, kl)
            want_cut = capi.components(ci, cx)
            got_cut = capi.mst_cut(got, n, t)
            assert all(np.array_equal(x, y) for x, y in zip(got_cut, want_cut)), (g, n, t)
        several += 1 < len(capi.mst_cut(got, n, 0.0)[1]) < n
        check_linkage(got, n)
    assert tied >= 120 and several >= 60 and cycles >= 100, (tied, several, cycles)


def check_linkage(edges, n):
    merges = capi.mst_linkage(edges, n)
    assert len(merges) == len(edges) and np.array_equal(merges["score"].view(np.uint32), edges["score"].view(np.uint32))
    members = {r: [r] for r in range(n)}
    for m, (left, right, _, size) in enumerate(merges.tolist()):
        assert left in members and right in members and left != right, "each cluster is merged once"
        L, R = members.pop(left), members.pop(right)
        assert min(L) < min(R), "left holds the smaller smallest row"
        assert (int(edges[m]["a"]) in L and int(edges[m]["b"]) in R) or (int(edges[m]["a"]) in R and int(edges[m]["b"]) in L)
        assert size == len(L) + len(R)
        members[n + m] = L + R
    return merges


def test_merge_heights_equal_scipys_single_linkage():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(77)
    for g in range(20):
        n = int(rng.integers(2, 60))
        # a complete graph: scipy's linkage joins everything
        S = rng.choice(np.array([.125, .25, .5, .625, .75, 1.0], F), (n, n))
        S = np.triu(S, 1) + np.triu(S, 1).T
        a, b = np.triu_indices(n, 1)
        edges = capi.mst(*csr(n, both_ways(zip(a.tolist(), b.tolist(), S[a, b].tolist()))))
        assert len(edges) == n - 1
        merges = check_linkage(edges, n)
        assert merges["size"][-1] == n
        Z = hierarchy.linkage(1.0 - S[a, b].astype(np.float64), "single")
        assert np.array_equal(np.sort(1.0 - merges["score"].astype(np.float64)), np.sort(Z[:, 2])), g
        # (heights only: the order among ties, and with it the sizes along the way, is ours)


def edge_array(rows):
    return np.array(rows, capi.MST_EDGE_DTYPE)


def test_malformed_input_is_invalid():
    L = capi.load()
    ne = C.c_uint64(5)
    out = np.zeros(8, capi.MST_EDGE_DTYPE)

    def raw(indptr, indices, scores, n, null_edges=False):
        indptr, indices, scores = np.ascontiguousarray(indptr, np.uint64), np.ascontiguousarray(indices, np.uint32), np.ascontiguousarray(scores, F)
        return L.gsim_mst(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), indices.ctypes.data_as(C.POINTER(C.c_uint32)) if len(indices) else None,
                          scores.ctypes.data_as(C.POINTER(C.c_float)) if len(scores) else None, n, None if null_edges else out.ctypes.data,
                          C.byref(ne))

    for what, args in {
        "indptr not starting at 0": ([1, 2, 2], [0, 1], [.5, .5], 2), "indptr decreasing": ([0, 2, 1], [1, 0], [.5, .5], 2),
        "a column outside the graph": ([0, 1, 2], [1, 2], [.5, .5], 2), "NULL indices": ([0, 1, 2], [], [.5, .5], 2),
        "NULL scores": ([0, 1, 2], [1, 0], [], 2), "a NaN score": ([0, 1, 2], [1, 0], [.5, float("nan")], 2),
        "NULL edges": ([0, 1, 2], [1, 0], [.5, .5], 2, True),
    }.items():
        assert raw(*args) == INVALID and len(message()) > 0 and ne.value == 0, what
    assert L.gsim_mst(None, None, None, 0, None, C.byref(ne)) == INVALID
    assert raw([0], [], [], 0) == OK and ne.value == 0, "no rows: legal"
    assert raw([0, 0], [], [], 1, True) == OK and ne.value == 0, "one row needs no edge buffer"
    assert len(capi.mst([0], [], [])) == 0
    # linkage and cut
    good = edge_array([(0, 1, .5), (1, 2, .25)])
    assert len(capi.mst_linkage(good, 3)) == 2 and len(capi.mst_linkage([], 0)) == 0 and len(capi.mst_linkage([], 5)) == 0
    for what, (rows, n) in {
        "a == b": ([(1, 1, .5)], 3), "a > b": ([(2, 1, .5)], 3), "b outside": ([(0, 3, .5)], 3), "a NaN score": ([(0, 1, float("nan"))], 3),
        "scores that increase": ([(0, 1, .25), (1, 2, .5)], 3), "a cycle": ([(0, 1, .5), (1, 2, .5), (0, 2, .5)], 4),
        "a repeated edge": ([(0, 1, .5), (0, 1, .5)], 3), "too many edges": ([(0, 1, .5), (0, 1, .5)], 2),
    }.items():
        with pytest.raises(capi.GsimError) as e:
            capi.mst_linkage(edge_array(rows), n)
        assert e.value.code == INVALID and len(str(e.value)) > 0, what
    for what, (rows, n, t) in {
        "a == b": ([(1, 1, .5)], 3, .5), "b outside": ([(0, 3, .5)], 3, .5), "a NaN threshold": ([(0, 1, .5)], 3, float("nan")),
    }.items():
        with pytest.raises(capi.GsimError) as e:
            capi.mst_cut(edge_array(rows), n, t)
        assert e.value.code == INVALID, what
    assert capi.mst_cut(edge_array([(0, 1, .5), (1, 2, .5), (0, 2, .5)]), 3, .5)[0].tolist() == [0, 0, 0], "a cycle is harmless to a cut"
    assert all(len(x) == 0 for x in capi.mst_cut([], 0, .5))
    nc = C.c_uint64(0)
    assert L.gsim_mst_cut(None, 0, 3, .5, None, None, None, C.byref(nc)) == INVALID
    assert L.gsim_mst_cut(None, 1, 3, .5, out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, C.byref(nc)) == INVALID
    assert L.gsim_mst_linkage(good.ctypes.data, 2, 3, None) == INVALID
