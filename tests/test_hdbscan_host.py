"""CPU checks of HDBSCAN's five calls -- gsim_db_core_scores, gsim_db_mreach_mst, gsim_db_hdbscan and the host companions
gsim_mreach_mst and gsim_mst_hdbscan: the symbols exist, the structs match the header, every argument error is reported before any
device state -- on a table that is not on a GPU -- with a message, a valid call on such a table is a state error (never a host
computation), and the two host functions against the Python restatement of the rule (hdbscan_rule.py): 200 random symmetric graphs
of at most 60 rows whose scores are drawn from at most six values (ties dominate), min_pts 1 to 5 (min_pts 1 equals gsim_mst),
min_cluster_size 2 to 6, excess of mass, leaves and NO_ROOTS; and hand-worked forests with dyadic scores, where double arithmetic is
exact: a three-way split at one level, small pieces that leave at the level of a split, two single rows tied with a large child, an
exact tie stability == sub (the parent wins), several trees with one below min_cluster_size, and 0, 1 and 2 rows.
tests/cpp/hdbscan_host_check.cpp, a stand-alone program over the two host functions with buffers of exactly the promised sizes, is
built plainly and run.  Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more (as tests/test_components_host.py says)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusimilarity_amd import capi
from hdbscan_rule import EOM, LEAF, NO_ROOTS, NOISE, hdbscan_rule, mreach_rule, tied
from test_mst_host import both_ways, csr, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32
NEW = ["gsim_db_core_scores", "gsim_db_mreach_mst", "gsim_db_hdbscan", "gsim_mreach_mst", "gsim_mst_hdbscan"]
FLAGS = (EOM, LEAF, EOM | NO_ROOTS, LEAF | NO_ROOTS)


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.Table.core_scores and capi.Table.mreach_mst and capi.Table.hdbscan and capi.mreach_mst and capi.mst_hdbscan


def test_structs_and_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    assert struct_fields(text, "gsim_mreach_stats") == [("gsim_mst_stats", "mst"), ("uint64_t", "core_launches"), ("uint64_t", "core_inserts"),
                                                        ("uint64_t", "core_rows"), ("double", "core_kernel_ms"), ("double", "core_tail_ms")]
    assert [n for n, _ in capi.GsimMreachStats._fields_] == ["mst", "core_launches", "core_inserts", "core_rows", "core_kernel_ms", "core_tail_ms"]
    assert capi.GsimMreachStats._fields_[0][1] is capi.GsimMstStats
    assert C.sizeof(capi.GsimMreachStats) == C.sizeof(capi.GsimMstStats) + 5 * 8
    assert struct_fields(text, "gsim_hdbscan_stats") == [("gsim_mreach_stats", "forest"), ("uint64_t", "clusters"), ("uint64_t", "noise"),
                                                         ("double", "select_ms"), ("double", "wall_ms")]
    assert [n for n, _ in capi.GsimHdbscanStats._fields_] == ["forest", "clusters", "noise", "select_ms", "wall_ms"]
    assert C.sizeof(capi.GsimHdbscanStats) == C.sizeof(capi.GsimMreachStats) + 4 * 8
    for name, value in (("NOISE", "0xFFFFFFFFu"), ("EOM", "0u"), ("LEAF", "1u"), ("NO_ROOTS", "2u")):
        assert re.search(r"#define\s+GSIM_HDBSCAN_%s\s+%s\b" % (name, value), text), name
        assert getattr(capi, "HDBSCAN_" + name) == int(value.rstrip("u"), 0)
    assert (NOISE, EOM, LEAF, NO_ROOTS) == (capi.HDBSCAN_NOISE, capi.HDBSCAN_EOM, capi.HDBSCAN_LEAF, capi.HDBSCAN_NO_ROOTS)
    assert re.search(r"#define\s+GSIM_KNN_MAX_K\s+128u\b", text)


class Calls:
    """the three device calls on a table that is not on a GPU, one argument changed at a time"""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        n = max(rows, 2)
        self.edges = np.zeros(n, capi.MST_EDGE_DTYPE)
        self.core = np.zeros(n, F)
        self.label = np.zeros(n, np.uint32)
        self.nedges, self.ncl = C.c_uint64(77), C.c_uint64(77)

    def core_scores(self, db=True, min_pts=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, core=True, **_):
        return capi.load().gsim_db_core_scores(self.t._h if db else None, min_pts, cutoff, metric, alpha, beta,
                                               capi._f32(self.core) if core else None, None)

    def mreach_mst(self, db=True, min_pts=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, edges=True, nedges=True, core=True, **_):
        self.nedges.value = 77
        return capi.load().gsim_db_mreach_mst(self.t._h if db else None, min_pts, cutoff, metric, alpha, beta,
                                              self.edges.ctypes.data if edges else None, C.byref(self.nedges) if nedges else None,
                                              capi._f32(self.core) if core else None, None)

    def hdbscan(self, db=True, min_pts=5, mcs=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0, label=True, ncl=True, **_):
        self.ncl.value = 77
        return capi.load().gsim_db_hdbscan(self.t._h if db else None, min_pts, mcs, cutoff, metric, alpha, beta, flags,
                                           capi._u32(self.label) if label else None, C.byref(self.ncl) if ncl else None, None, None, None, None,
                                           None, None)

    def all(self):
        return (("core_scores", self.core_scores), ("mreach_mst", self.mreach_mst), ("hdbscan", self.hdbscan))


def test_argument_errors_come_before_any_device_state():
    call = Calls()
    inf, nan = float("inf"), float("nan")
    shared = {
        "NULL db": dict(db=False), "min_pts 0": dict(min_pts=0), "min_pts 130": dict(min_pts=130), "min_pts 2^32 - 1": dict(min_pts=0xFFFFFFFF),
        "cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff NaN": dict(cutoff=nan),
        "cutoff inf": dict(cutoff=inf), "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
        "asymmetric weights": dict(metric=TV, alpha=0.3, beta=0.7), "negative weights": dict(metric=TV, alpha=-0.5, beta=-0.5),
        "infinite weights": dict(metric=TV, alpha=inf, beta=inf), "NaN weights": dict(metric=TV, alpha=nan, beta=nan),
    }
    own = {
        "core_scores": {"NULL core": dict(core=False)},
        "mreach_mst": {"NULL edges": dict(edges=False), "NULL nedges": dict(nedges=False)},
        "hdbscan": {"NULL label_of": dict(label=False), "NULL nclusters": dict(ncl=False), "min_cluster_size 0": dict(mcs=0),
                    "min_cluster_size 1": dict(mcs=1), "unknown flags": dict(flags=4), "all flag bits": dict(flags=0xFFFFFFFF)},
    }
    for name, fn in call.all():
        for what, kw in list(shared.items()) + list(own[name].items()):
            assert fn(**kw) == INVALID, (name, what)
            assert len(message()) > 0, (name, what)
        assert fn(min_pts=129) == STATE and fn(min_pts=1) == STATE, (name, "the largest and the smallest min_pts are legal")
    assert call.mreach_mst(cutoff=2.0) == INVALID and call.nedges.value == 0
    assert call.hdbscan(cutoff=2.0) == INVALID and call.ncl.value == 0
    assert call.mreach_mst(core=False) == STATE, "core is optional there"
    call.t.close()
    wide = Calls(bits=4128, rows=3)
    for name, fn in wide.all():
        assert fn() == INVALID and "4096" in message(), name
    wide.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Calls()
    tiny = float(np.nextafter(F(0), F(1)))
    for name, fn in call.all():
        for kw in (dict(), dict(cutoff=1.0), dict(cutoff=tiny), dict(metric=TV, alpha=0.5, beta=0.5), dict(flags=3, mcs=2)):
            assert fn(**kw) == STATE, (name, kw)
            assert "GPU" in message(), (name, kw)
        assert fn(cutoff=2.0) == INVALID, "an argument error wins over it"
    assert call.nedges.value == 0 and call.ncl.value == 0
    call.t.close()
    empty = Calls(rows=0)
    for name, fn in empty.all():
        assert fn() == OK, name
        assert fn(cutoff=0.0) == INVALID, "an argument error still wins"
    assert empty.core_scores(core=False) == OK and empty.mreach_mst(edges=False) == OK and empty.hdbscan(label=False) == OK
    assert empty.nedges.value == 0 and empty.ncl.value == 0
    edges, core, st = empty.t.mreach_mst(5, 0.5)
    assert len(edges) == 0 and len(core) == 0 and st["rows"] == st["edges"] == st["core_launches"] == 0
    out = empty.t.hdbscan(5, 5, 0.5)
    assert all(len(x) == 0 for x in out[:6]) and out[6]["clusters"] == 0
    assert len(empty.t.core_scores(5, 0.5)[0]) == 0
    empty.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    for fn in (lambda: t.core_scores(3, 0.5), lambda: t.mreach_mst(3, 0.5), lambda: t.hdbscan(3, 2, 0.5)):
        with pytest.raises(capi.GsimError) as e:
            fn()
        assert e.value.code == STATE and len(str(e.value)) > 0
    t.close()


def random_graph(rng):
    """-> (n, S): S symmetric float32 with at most six distinct positive values; 0: the pair is not listed"""
    n = int(rng.integers(0, 61))
    values = rng.choice(np.array([.125, .25, .5, .625, .75, 1.0], F), int(rng.integers(1, 7)), replace=False)
    density = float(rng.choice([0.0, 1.5 / max(n, 1), 3.0 / max(n, 1), 0.1, 0.3, 0.6]))
    U = np.triu(np.where(rng.random((n, n)) < density, rng.choice(values, (n, n)), 0).astype(F), 1)
    return n, U + U.T


def listed(S, rng):
    a, b = np.nonzero(np.triu(S, 1))
    entries = both_ways(zip(a.tolist(), b.tolist(), S[a, b].tolist()))
    return csr(len(S), [entries[k] for k in rng.permutation(len(entries))])


def same_selection(got, want, what):
    label, leave, first_row, sizes, birth, stability = got
    assert label.tobytes() == want["label"].tobytes(), (what, label, want["label"])
    assert leave.tobytes() == want["leave"].tobytes(), (what, leave, want["leave"])
    assert first_row.tobytes() == want["first_row"].tobytes() and sizes.tobytes() == want["sizes"].tobytes(), (what, first_row, sizes)
    assert birth.tobytes() == want["birth"].tobytes(), (what, birth, want["birth"])
    assert len(stability) == len(want["stability"])
    for x, y in zip(stability.tolist(), want["stability"]):
        assert abs(x - float(y)) <= 1e-12 * float(y), (what, x, y)


def test_the_host_functions_equal_the_rule_on_random_graphs_full_of_ties():
    rng = np.random.default_rng(0x4DB5)
    floor = 0.0625  # below every score
    ties = capped = several = noisy = parents = splits = 0
    for g in range(200):
        n, S = random_graph(rng)
        graph = listed(S, rng)
        plain = capi.mst(*graph)
        for min_pts in range(1, 6):
            want, want_core = mreach_rule(S, floor, min_pts)
            got, core = capi.mreach_mst(*graph, min_pts)
            assert got.tobytes() == want.tobytes(), (g, n, min_pts, got, want)
            assert core.tobytes() == want_core.tobytes(), (g, n, min_pts)
            if min_pts == 1:
                assert got.tobytes() == plain.tobytes(), (g, n)
            ties += tied(got) * 2 >= len(got) > 0
            capped += len(got) > 0 and min_pts > 1 and got.tobytes() != plain.tobytes()
            mcs = 2 + (g + min_pts) % 5
            for flags in FLAGS:
                rule = hdbscan_rule(want, n, floor, mcs, flags)
                same_selection(capi.mst_hdbscan(got, n, floor, mcs, flags), rule, (g, n, min_pts, mcs, flags))
                several += len(rule["sizes"]) >= 2
                noisy += 0 < int((rule["label"] == NOISE).sum()) < n
                if flags == EOM:
                    splits += len(rule["all_stability"]) > len(rule["sizes"]) >= 2
                    parents += len(rule["all_stability"]) >= 3 and len(rule["sizes"]) == 1
    assert ties >= 300 and capped >= 200 and several >= 300 and noisy >= 500 and parents >= 20 and splits >= 20, \
        (ties, capped, several, noisy, parents, splits)


def edge_array(rows):
    return np.array(rows, capi.MST_EDGE_DTYPE)


def select(edges, n, floor, mcs, flags=EOM):
    """both the library's answer and the rule's must be the hand-worked one: the library's is returned as lists"""
    edges = edge_array(edges)
    got = capi.mst_hdbscan(edges, n, floor, mcs, flags)
    same_selection(got, hdbscan_rule(edges, n, floor, mcs, flags), (n, floor, mcs, flags))
    return [x.tolist() for x in got]


THREE = [(0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 8)]  # three chains of three rows


def test_a_three_way_split_at_one_level():
    """three chains at 1.0 joined at .5 by two edges: ONE node at .5 with three large children, not two binary merges"""
    edges = [(a, b, 1.0) for a, b in THREE] + [(2, 3, .5), (5, 6, .5)]
    # the root lives from .25 to .5 with 9 rows: 2.25; each child from .5 to 1.0 with 3 rows: 1.5, together 4.5: the children win
    for flags in FLAGS:
        label, leave, first, sizes, birth, stab = select(edges, 9, .25, 3, flags)
        assert label == [0, 0, 0, 1, 1, 1, 2, 2, 2] and leave == [1.0] * 9 and first == [0, 3, 6] and sizes == [3, 3, 3]
        assert birth == [.5, .5, .5] and stab == [1.5, 1.5, 1.5]
    # with min_cluster_size 4 no child is large: the root ends at .5 and is a cluster without child clusters
    for flags in FLAGS:
        label, leave, first, sizes, birth, stab = select(edges, 9, .25, 4, flags)
        assert label == [0] * 9 and leave == [.5] * 9 and (first, sizes, birth, stab) == ([0], [9], [.25], [2.25])


def test_an_exact_tie_selects_the_parent():
    edges = [(a, b, 1.0) for a, b in THREE] + [(2, 3, .5), (5, 6, .5)]
    # born at 0: the root's 9 x .5 = 4.5 equals its children's 3 x 1.5
    label, leave, first, sizes, birth, stab = select(edges, 9, 0.0, 3)
    assert label == [0] * 9 and leave == [1.0] * 9 and (first, sizes, birth, stab) == ([0], [9], [0.0], [4.5])
    # ... unless roots are not wanted, or only leaves are
    for flags in (EOM | NO_ROOTS, LEAF, LEAF | NO_ROOTS):
        label, _, first, sizes, birth, stab = select(edges, 9, 0.0, 3, flags)
        assert label == [0, 0, 0, 1, 1, 1, 2, 2, 2] and (first, sizes, birth, stab) == ([0, 3, 6], [3, 3, 3], [.5] * 3, [1.5] * 3)
    # a tie one level down: chains at .75 under a split at .5, born at .25: 9 x .25 = 3 x (3 x .25)
    lower = [(a, b, .75) for a, b in THREE] + [(2, 3, .5), (5, 6, .5)]
    label, _, first, sizes, birth, stab = select(lower, 9, .25, 3)
    assert label == [0] * 9 and (first, sizes, birth, stab) == ([0], [9], [.25], [2.25])
    # and a parent that wins outright
    label, _, first, sizes, birth, stab = select(lower, 9, 0.0, 3)
    assert label == [0] * 9 and (first, sizes, birth, stab) == ([0], [9], [0.0], [4.5])


def test_small_pieces_leave_at_the_level_of_a_split():
    """the three-way split, and at the same level .5: the single rows 9 and 10 and the pair 11 - 12 (joined at .75: a node of two rows,
    smaller than min_cluster_size).  They leave the root at .5 -- the pair too, not at .75 -- and belong to no child"""
    edges = [(a, b, 1.0) for a, b in THREE] + [(11, 12, .75), (0, 10, .5), (2, 3, .5), (5, 6, .5), (8, 9, .5), (10, 11, .5)]
    label, leave, first, sizes, birth, stab = select(edges, 13, .25, 3)
    # root: 13 x .25 = 3.25 against 4.5
    assert label == [0, 0, 0, 1, 1, 1, 2, 2, 2, NOISE, NOISE, NOISE, NOISE] and leave == [1.0] * 9 + [.5] * 4
    assert (first, sizes, birth, stab) == ([0, 3, 6], [3, 3, 3], [.5] * 3, [1.5] * 3)
    # born at 0 the root wins, 6.5 against 4.5, and takes the small pieces with it
    label, leave, first, sizes, birth, stab = select(edges, 13, 0.0, 3)
    assert label == [0] * 13 and leave == [1.0] * 9 + [.5] * 4 and (first, sizes, birth, stab) == ([0], [13], [0.0], [6.5])


def test_two_single_rows_tied_with_a_large_child():
    """0 - 1 - 2 - 3 at 1.0; rows 4 and 5 join them at .5: one large child, so the cluster goes on as that child"""
    edges = [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0), (3, 4, .5), (3, 5, .5)]
    for flags in FLAGS:  # (a root without child clusters is selected whatever the flags say)
        label, leave, first, sizes, birth, stab = select(edges, 6, .25, 3, flags)
        # 2 rows x (.5 - .25) + 4 rows x (1 - .25)
        assert label == [0] * 6 and leave == [1.0] * 4 + [.5] * 2 and (first, sizes, birth, stab) == ([0], [6], [.25], [3.5])


def test_a_forest_of_several_trees():
    """the tree above; 6 - 7, a tree below min_cluster_size; row 8 alone; 9 - 10 - 11 at .75"""
    edges = [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0), (6, 7, 1.0), (9, 10, .75), (10, 11, .75), (3, 4, .5), (3, 5, .5)]
    label, leave, first, sizes, birth, stab = select(edges, 12, .25, 3)
    assert label == [0] * 6 + [NOISE] * 3 + [1] * 3 and leave == [1.0] * 4 + [.5] * 2 + [0.0] * 3 + [.75] * 3
    assert (first, sizes, birth, stab) == ([0, 9], [6, 3], [.25, .25], [3.5, 1.5])
    # with min_cluster_size 2 the pair is a cluster too, between the others in the numbering
    label, _, first, sizes, _, stab = select(edges, 12, .25, 2)
    assert label == [0] * 6 + [1, 1, NOISE] + [2] * 3 and first == [0, 6, 9] and sizes == [6, 2, 3] and stab == [3.5, 1.5, 1.5]


def test_no_rows_one_row_two_rows_and_no_edges():
    for n in (0, 1, 2, 7):
        label, leave, first, sizes, birth, stab = select([], n, .5, 2)
        assert label == [NOISE] * n and leave == [0.0] * n and first == sizes == birth == stab == []
    label, leave, first, sizes, birth, stab = select([(0, 1, 1.0)], 2, .5, 2)
    assert label == [0, 0] and leave == [1.0, 1.0] and (first, sizes, birth, stab) == ([0], [2], [.5], [1.0])
    label, leave, _, _, _, _ = select([(0, 1, 1.0)], 2, .5, 3)
    assert label == [NOISE] * 2 and leave == [0.0] * 2
    # a forest whose every edge sits at the floor: born and ended at the same level
    label, leave, first, sizes, birth, stab = select([(0, 1, .5), (1, 2, .5)], 3, .5, 2)
    assert label == [0] * 3 and leave == [.5] * 3 and (sizes, birth, stab) == ([3], [.5], [0.0])
    # gsim_mreach_mst: no rows, one row, two rows
    assert [len(x) for x in capi.mreach_mst([0], [], [], 3)] == [0, 0]
    edges, core = capi.mreach_mst([0, 0], [], [], 1)
    assert len(edges) == 0 and core.tolist() == [1.0]
    assert capi.mreach_mst([0, 0], [], [], 2)[1].tolist() == [0.0]
    edges, core = capi.mreach_mst([0, 1, 2], [1, 0], [.5, .5], 2)
    assert edges.tolist() == [(0, 1, .5)] and core.tolist() == [.5, .5]
    edges, core = capi.mreach_mst([0, 1, 2], [1, 0], [.5, .5], 3)
    assert len(edges) == 0 and core.tolist() == [0.0, 0.0]


def test_malformed_input_is_invalid():
    L = capi.load()
    good = edge_array([(0, 1, .5), (1, 2, .25)])
    assert [x.tolist() for x in capi.mst_hdbscan(good, 3, .25, 2)[:2]] == [[0, 0, 0], [.5, .5, .25]]
    nan = float("nan")
    for what, (rows, n, floor, mcs, flags) in {
        "a == b": ([(1, 1, .5)], 3, .25, 2, 0), "a > b": ([(2, 1, .5)], 3, .25, 2, 0), "b outside": ([(0, 3, .5)], 3, .25, 2, 0),
        "a NaN score": ([(0, 1, nan)], 3, .25, 2, 0), "scores that increase": ([(0, 1, .25), (1, 2, .5)], 3, .25, 2, 0),
        "a cycle": ([(0, 1, .5), (1, 2, .5), (0, 2, .5)], 4, .25, 2, 0), "a repeated edge": ([(0, 1, .5), (0, 1, .5)], 3, .25, 2, 0),
        "too many edges": ([(0, 1, .5), (0, 1, .5)], 2, .25, 2, 0), "a floor above an edge": ([(0, 1, .5), (1, 2, .25)], 3, .375, 2, 0),
        "a floor above all": ([(0, 1, .5)], 3, 1.0, 2, 0), "a NaN floor": ([(0, 1, .5)], 3, nan, 2, 0),
        "min_cluster_size 1": ([(0, 1, .5)], 3, .25, 1, 0), "min_cluster_size 0": ([(0, 1, .5)], 3, .25, 0, 0),
        "unknown flags": ([(0, 1, .5)], 3, .25, 2, 4), "a NaN floor without edges": ([], 3, nan, 2, 0),
    }.items():
        with pytest.raises(capi.GsimError) as e:
            capi.mst_hdbscan(edge_array(rows), n, floor, mcs, flags)
        assert e.value.code == INVALID and len(str(e.value)) > 0, what
    ncl = C.c_uint64(5)
    label = np.zeros(3, np.uint32)
    assert L.gsim_mst_hdbscan(good.ctypes.data, 2, 3, .25, 2, 0, capi._u32(label), None, None, None, None, None, None) == INVALID
    assert L.gsim_mst_hdbscan(good.ctypes.data, 2, 3, .25, 2, 0, None, C.byref(ncl), None, None, None, None, None) == INVALID and ncl.value == 0
    assert L.gsim_mst_hdbscan(None, 2, 3, .25, 2, 0, capi._u32(label), C.byref(ncl), None, None, None, None, None) == INVALID
    assert L.gsim_mst_hdbscan(good.ctypes.data, 2, 3, .25, 2, 0, capi._u32(label), C.byref(ncl), None, None, None, None, None) == OK
    assert ncl.value == 1 and label.tolist() == [0, 0, 0], "every optional output may be NULL"
    assert L.gsim_mst_hdbscan(None, 0, 0, .25, 2, 0, None, C.byref(ncl), None, None, None, None, None) == OK and ncl.value == 0
    # gsim_mreach_mst: gsim_mst's checks, and min_pts
    ne = C.c_uint64(5)
    out = np.zeros(8, capi.MST_EDGE_DTYPE)
    core = np.zeros(8, F)

    def raw(indptr, indices, scores, n, min_pts=2, null_edges=False, null_core=False):
        indptr, indices, scores = np.ascontiguousarray(indptr, np.uint64), np.ascontiguousarray(indices, np.uint32), np.ascontiguousarray(scores, F)
        return L.gsim_mreach_mst(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), capi._u32(indices) if len(indices) else None,
                                 capi._f32(scores) if len(scores) else None, n, min_pts, None if null_edges else out.ctypes.data, C.byref(ne),
                                 None if null_core else capi._f32(core))

    for what, args in {
        "indptr not starting at 0": ([1, 2, 2], [0, 1], [.5, .5], 2), "indptr decreasing": ([0, 2, 1], [1, 0], [.5, .5], 2),
        "a column outside the graph": ([0, 1, 2], [1, 2], [.5, .5], 2), "NULL indices": ([0, 1, 2], [], [.5, .5], 2),
        "NULL scores": ([0, 1, 2], [1, 0], [], 2), "a NaN score": ([0, 1, 2], [1, 0], [.5, nan], 2),
        "NULL edges": ([0, 1, 2], [1, 0], [.5, .5], 2, 2, True), "min_pts 0": ([0, 1, 2], [1, 0], [.5, .5], 2, 0),
    }.items():
        assert raw(*args) == INVALID and len(message()) > 0 and ne.value == 0, what
    assert L.gsim_mreach_mst(None, None, None, 0, 2, None, C.byref(ne), None) == INVALID
    assert raw([0, 1, 2], [1, 0], [.5, .5], 2, 2, False, True) == OK and ne.value == 1, "core is optional"
    assert raw([0, 1, 2], [1, 0], [.5, .5], 2, 1000) == OK and ne.value == 0, "any min_pts >= 1 is legal on the host"
    assert raw([0], [], [], 0) == OK and ne.value == 0, "no rows: legal"
    assert raw([0, 0], [], [], 1, 2, True) == OK, "one row needs no edge buffer"
    with pytest.raises(capi.GsimError):
        capi.mreach_mst([0, 1, 2], [1, 0], [.5], 2)


def test_the_stand_alone_checker_builds_plainly_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "hdbscan_host_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "hdbscan_host_check")
    libdir = os.path.join(ROOT, "gpusimilarity_amd")
    deps = [src, os.path.join(ROOT, "include", "gpusim_hip.h"), os.path.join(libdir, "libgsim_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + libdir, "-lgsim_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout + r.stderr
