"""The case list of the clustering fronts that came after the single-table list, recorded by scripts/make_front_errors_golden.py
(list "cluster") and replayed by tests/test_cluster_front_errors_host.py: gsim_db_dbscan, gsim_db_core_scores, gsim_db_mreach_mst,
gsim_db_hdbscan, gsim_db_label_sums, gsim_labelset_create, gsim_db_search_labels, gsim_db_linkage, gsim_db_snn and
gsim_db_jarvis_patrick on tables that are not on a GPU -- one argument changed at a time from a valid call, and a handful of valid
calls (a state error: the tables have no rows on a GPU; GSIM_OK where the call answers without one) -- and the host functions
gsim_dbscan, gsim_mreach_mst, gsim_mst_hdbscan, gsim_linkage, gsim_snn and gsim_jarvis_patrick on host arrays, whose valid cases
record the result arrays.  `run_all()` returns {case id: {code, message, out}} in the shape of single_front_errors_cases.py.

A label set cannot be made without a GPU.  gsim_db_search_labels reads its owner before any device state, so the cases pass a
stand-in: zeroed memory that begins as gsim_labelset does (capi_internal.h), with the owner and the row count the case asks for."""
import ctypes as C

import numpy as np

import single_front_errors_cases as single
from front_errors_cases import CUTOFF, K, METRIC, NULL_GRAPH, VALID_CUTOFF, VALID_K, VALID_METRIC, host_table, merged
from gpusimilarity_amd import capi
from single_front_errors_cases import FP, METRICS, RANGE, ROWS, TAN, TV, U32P, U64P, nulls

inf, nan = float("inf"), float("nan")
F64P = C.POINTER(C.c_double)
NONE = capi.LABEL_NONE


class FakeLabelset(C.Structure):
    _fields_ = [("owner", C.c_void_p), ("device", C.c_int), ("nrows", C.c_uint64), ("nlabels", C.c_uint32), ("rest", C.c_uint8 * 256)]


class Calls(single.Calls):
    """The ten entry points on one host table, every argument with a valid default (the helpers are single_front_errors_cases.Calls')."""

    def labelset(self, ls):
        """None, or a stand-in label set: "mine" (owner: the table), "other" (another handle), "stale" (the table, another row count)"""
        if ls is None:
            return None
        f = FakeLabelset()
        f.owner = (self.other if ls == "other" else self.t)._h.value
        f.nrows = self.rows + (5 if ls == "stale" else 0)
        f.nlabels = 3
        self.keep.append(f)
        return C.cast(C.byref(f), C.c_void_p)

    def fit_labels(self, labels, n):
        return np.arange(max(n, 0) if n <= 10 * ROWS else 0) % 3 if isinstance(labels, str) else labels

    def dbscan(self, db=True, cutoff=0.5, min_pts=3, metric=TAN, alpha=1.0, beta=1.0, label_of=True, nclusters=True, degree=True, anchor=True,
               first_row=True, sizes=True, stats=True):
        n = 4 * self.rows
        return self.seen(capi.load().gsim_db_dbscan(
            self.db(db), cutoff, min_pts, metric, alpha, beta, self.out("label_of", label_of, n), self.out("nclusters", nclusters, 4),
            self.out("degree", degree, n), self.out("anchor", anchor, n), self.out("first_row", first_row, n), self.out("sizes", sizes, n),
            self.stats(capi.GsimDbscanStats, stats)))

    def core_scores(self, db=True, min_pts=3, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, core=True, stats=True):
        return self.seen(capi.load().gsim_db_core_scores(self.db(db), min_pts, cutoff, metric, alpha, beta, self.out("core", core, 4 * self.rows, FP),
                                                         self.stats(capi.GsimKnnStats, stats)))

    def mreach_mst(self, db=True, min_pts=3, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, edges=True, nedges=True, core=True, stats=True):
        return self.seen(capi.load().gsim_db_mreach_mst(
            self.db(db), min_pts, cutoff, metric, alpha, beta, self.out("edges", edges, 12 * self.rows, None), self.out("nedges", nedges, 8, U64P),
            self.out("core", core, 4 * self.rows, FP), self.stats(capi.GsimMreachStats, stats)))

    def hdbscan(self, db=True, min_pts=3, min_cluster_size=2, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0, label_of=True, nclusters=True,
                leave=True, first_row=True, sizes=True, birth=True, stability=True, stats=True):
        n = 4 * self.rows
        return self.seen(capi.load().gsim_db_hdbscan(
            self.db(db), min_pts, min_cluster_size, cutoff, metric, alpha, beta, flags, self.out("label_of", label_of, n),
            self.out("nclusters", nclusters, 8, U64P), self.out("leave", leave, n, FP), self.out("first_row", first_row, n), self.out("sizes", sizes, n),
            self.out("birth", birth, n, FP), self.out("stability", stability, 2 * n, F64P), self.stats(capi.GsimHdbscanStats, stats)))

    def label_sums(self, db=True, labels="fit", nlabels=3, row_begin=0, row_end=None, metric=TAN, alpha=1.0, beta=1.0, flags=0, launch_pairs=0,
                   own_q=True, other_label=True, other_q=True, sizes=True, stats=True):
        re = self.rows if row_end is None else row_end
        lab = self.fit_labels(labels, re - row_begin)
        return self.seen(capi.load().gsim_db_label_sums(
            self.db(db), self.inp(lab, np.uint32, U32P), nlabels, row_begin, re, metric, alpha, beta, flags, launch_pairs,
            self.out("own_q", own_q, 8 * self.rows, U64P), self.out("other_label", other_label, 4 * self.rows),
            self.out("other_q", other_q, 8 * self.rows, U64P), self.out("sizes", sizes, 4 * 3), self.stats(capi.GsimLabelSumsStats, stats)))

    def labelset_create(self, db=True, labels="fit", nlabels=3, out=True):
        lab = self.inp(self.fit_labels(labels, self.rows), np.uint32, U32P)
        return self.graph(lambda o: capi.load().gsim_labelset_create(self.db(db), lab, nlabels, o), out)

    def search_labels(self, db=True, ls="mine", queries=True, nq=2, k=3, cutoff=0.0, metric=TAN, alpha=1.0, beta=1.0, launch_rows=0, hits=True,
                      hit_labels=True, counts=True, stats=True):
        q = self.inp(np.ones((2, self.W)), np.uint32, U32P) if queries else None
        return self.seen(capi.load().gsim_db_search_labels(
            self.db(db), self.labelset(ls), q, nq, k, cutoff, metric, alpha, beta, launch_rows, self.out("hits", hits, 12 * 2 * 3, None),
            self.out("hit_labels", hit_labels, 4 * 2 * 3), self.out("counts", counts, 4 * 2), self.out("approx", True, 8 * 2, U64P),
            self.out("rows_kept", True, 8 * 2, U64P), self.out("label_best", True, 12 * 2 * 3, None), self.out("label_kept", True, 4 * 2 * 3),
            self.stats(capi.GsimLabelSearchStats, stats)))

    def linkage(self, db=True, row_begin=0, row_end=None, kind=capi.LINKAGE_COMPLETE, metric=TAN, alpha=1.0, beta=1.0, launch_steps=0, merges=True,
                nmerges=True, stats=True):
        re = self.rows if row_end is None else row_end
        return self.seen(capi.load().gsim_db_linkage(self.db(db), row_begin, re, kind, metric, alpha, beta, launch_steps,
                                                     self.out("merges", merges, 32 * ROWS, None), self.out("nmerges", nmerges, 8, U64P),
                                                     self.stats(capi.GsimLinkageStats, stats)))

    def snn(self, db=True, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0, out=True):
        return self.graph(lambda o: capi.load().gsim_db_snn(self.db(db), k, cutoff, metric, alpha, beta, flags, o), out)

    def jarvis_patrick(self, db=True, k=5, kmins=(1, 2, 4), nlevels=None, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0, cluster_of=True,
                       nclusters=True, first_row=True, sizes=True, stats=True):
        nl = (len(kmins) if kmins is not None else 1) if nlevels is None else nlevels
        n = 4 * 8 * self.rows
        return self.seen(capi.load().gsim_db_jarvis_patrick(
            self.db(db), k, self.inp(kmins, np.uint32, U32P), nl, cutoff, metric, alpha, beta, flags, self.out("cluster_of", cluster_of, n),
            self.out("nclusters", nclusters, 4 * 8), self.out("first_row", first_row, n), self.out("sizes", sizes, n),
            self.stats(capi.GsimSnnStats, stats)))


# ---- the host functions ----
# single_front_errors_cases' graph (a path 0-1-2, the pair 4-5, the lone rows 3 and 6) for gsim_dbscan and gsim_mreach_mst; the
# lists below for gsim_snn and gsim_jarvis_patrick: 0, 1, 2 name each other, 3 names 0 and 4, 4 names 3, 5 and 6 name nobody
GRAPH = single.GRAPH
LISTS = dict(indptr=(0, 2, 4, 6, 8, 9, 9, 9), indices=(1, 2, 0, 2, 0, 1, 0, 4, 3), nrows=7)
FOREST = ((1, 2, 0.75), (0, 1, 0.5), (4, 5, 0.25))  # gsim_mst's forest of GRAPH, in order E
MATRIX = ((1.0, 0.9, 0.2, 0.1), (0.9, 1.0, 0.3, 0.2), (0.2, 0.3, 1.0, 0.8), (0.1, 0.2, 0.8, 1.0))


class Graphs(single.Graphs):
    def dbscan(self, indptr=GRAPH["indptr"], indices=GRAPH["indices"], scores=GRAPH["scores"], nrows=GRAPH["nrows"], min_pts=2, label_of=True,
               anchor=True, first_row=True, sizes=True, nclusters=True):
        ip, ix, sc = self.csr(indptr, indices, scores)
        return self.seen(capi.load().gsim_dbscan(ip, ix, sc, nrows, min_pts, self.out("label_of", label_of, 4 * 7), self.out("anchor", anchor, 4 * 7),
                                                 self.out("first_row", first_row, 4 * 7), self.out("sizes", sizes, 4 * 7),
                                                 self.out("nclusters", nclusters, 8, U64P)))

    def mreach_mst(self, indptr=GRAPH["indptr"], indices=GRAPH["indices"], scores=GRAPH["scores"], nrows=GRAPH["nrows"], min_pts=2, edges=True,
                   nedges=True, core=True):
        ip, ix, sc = self.csr(indptr, indices, scores)
        return self.seen(capi.load().gsim_mreach_mst(ip, ix, sc, nrows, min_pts, self.out("edges", edges, 12 * 6, None),
                                                     self.out("nedges", nedges, 8, U64P), self.out("core", core, 4 * 7, FP)))

    def mst_hdbscan(self, edges=FOREST, nedges=None, nrows=GRAPH["nrows"], floor=0.25, min_cluster_size=2, flags=0, label_of=True, nclusters=True,
                    leave=True, first_row=True, sizes=True, birth=True, stability=True):
        e = None
        if edges is not None:
            e = np.array(list(edges), capi.MST_EDGE_DTYPE)
            self.keep.append(e)
        ne = (len(e) if e is not None else 0) if nedges is None else nedges
        return self.seen(capi.load().gsim_mst_hdbscan(
            e.ctypes.data if e is not None else None, ne, nrows, floor, min_cluster_size, flags, self.out("label_of", label_of, 4 * 7),
            self.out("nclusters", nclusters, 8, U64P), self.out("leave", leave, 4 * 7, FP), self.out("first_row", first_row, 4 * 7),
            self.out("sizes", sizes, 4 * 7), self.out("birth", birth, 4 * 7, FP), self.out("stability", stability, 8 * 7, F64P)))

    def linkage(self, scores=MATRIX, n=None, ld=None, kind=capi.LINKAGE_COMPLETE, merges=True, nmerges=True, scans=True):
        s = self.inp(scores, np.float32, FP)
        n = (len(scores) if scores is not None else 4) if n is None else n
        return self.seen(capi.load().gsim_linkage(s, n, n if ld is None else ld, kind, self.out("merges", merges, 32 * 3, None),
                                                  self.out("nmerges", nmerges, 8, U64P), self.out("scans", scans, 8, U64P)))

    def snn(self, indptr=LISTS["indptr"], indices=LISTS["indices"], nrows=LISTS["nrows"], flags=0, shared=True):
        ip, ix, _ = self.csr(indptr, indices)
        return self.seen(capi.load().gsim_snn(ip, ix, nrows, flags, self.out("shared", shared, 4 * 9)))

    def jarvis_patrick(self, indptr=LISTS["indptr"], indices=LISTS["indices"], nrows=LISTS["nrows"], kmins=(0, 1), nlevels=None, flags=0,
                       cluster_of=True, first_row=True, sizes=True, nclusters=True):
        ip, ix, _ = self.csr(indptr, indices)
        nl = (len(kmins) if kmins is not None else 1) if nlevels is None else nlevels
        return self.seen(capi.load().gsim_jarvis_patrick(
            ip, ix, nrows, self.inp(kmins, np.uint32, U32P), nl, flags, self.out("cluster_of", cluster_of, 4 * 8 * 7),
            self.out("first_row", first_row, 4 * 8 * 7), self.out("sizes", sizes, 4 * 8 * 7), self.out("nclusters", nclusters, 4 * 8)))


MIN_PTS = {"min_pts 0": dict(min_pts=0), "min_pts above the largest": dict(min_pts=capi.KNN_MAX_K + 2), "min_pts huge": dict(min_pts=0xFFFFFFFF),
           "valid min_pts 1": dict(min_pts=1), "valid min_pts largest": dict(min_pts=capi.KNN_MAX_K + 1)}
SELECTION = {"min_cluster_size 0": dict(min_cluster_size=0), "min_cluster_size 1": dict(min_cluster_size=1), "unknown flags": dict(flags=4),
             "all flags": dict(flags=0xFFFFFFFF), "valid leaf": dict(flags=capi.HDBSCAN_LEAF),
             "valid leaf without roots": dict(flags=capi.HDBSCAN_LEAF | capi.HDBSCAN_NO_ROOTS)}
LABELS = {"no labels": dict(nlabels=0), "NULL labels": dict(labels=None), "a label equal to nlabels": dict(labels=[0, 1, 3] + [0] * (ROWS - 3)),
          "valid unlabelled rows": dict(labels=[NONE] * ROWS)}
NO_STATS = {"valid without stats": dict(stats=False)}
# gsim_db_knn's checks of the lists as gsim_db_snn and gsim_db_jarvis_patrick make them
LISTS_FRONT = merged(METRIC, VALID_METRIC, CUTOFF, VALID_CUTOFF, K)

ENTRIES = {
    "dbscan": merged(nulls("db", "label_of", "nclusters"), METRICS, CUTOFF, VALID_CUTOFF, NO_STATS, {
        "min_pts 0": dict(min_pts=0), "valid min_pts 1": dict(min_pts=1), "valid min_pts huge": dict(min_pts=0xFFFFFFFF),
        "valid outputs not asked for": dict(degree=False, anchor=False, first_row=False, sizes=False)}),
    "core_scores": merged(nulls("db", "core"), METRICS, CUTOFF, VALID_CUTOFF, MIN_PTS, NO_STATS),
    "mreach_mst": merged(nulls("db", "edges", "nedges"), METRICS, CUTOFF, VALID_CUTOFF, MIN_PTS, NO_STATS, {"valid without core": dict(core=False)}),
    "hdbscan": merged(nulls("db", "label_of", "nclusters"), METRICS, CUTOFF, VALID_CUTOFF, MIN_PTS, SELECTION, NO_STATS, {
        "valid outputs not asked for": dict(leave=False, first_row=False, sizes=False, birth=False, stability=False)}),
    "label_sums": merged(nulls("db", "own_q", "other_label", "other_q"), METRIC, VALID_METRIC, RANGE, LABELS, NO_STATS, {
        "unknown flags": dict(flags=2), "all flags": dict(flags=0xFFFFFFFF), "valid own only": dict(flags=capi.LABEL_SUMS_OWN_ONLY),
        "valid own only without the others": dict(flags=capi.LABEL_SUMS_OWN_ONLY, other_label=False, other_q=False),
        "valid NULL labels on an empty range": dict(labels=None, row_begin=9, row_end=9), "valid without sizes": dict(sizes=False)}),
    "labelset_create": merged(NULL_GRAPH, LABELS, {"valid": dict()}),
    "search_labels": merged(nulls("db", "queries", "hits", "hit_labels", "counts"), METRIC, VALID_METRIC, NO_STATS, {
        "NULL ls": dict(ls=None), "a label set of another handle": dict(ls="other"), "valid stale label set": dict(ls="stale"),
        "valid NULL queries with nq 0": dict(queries=False, nq=0)}),
    "linkage": merged(nulls("db", "merges", "nmerges"), METRICS, RANGE, NO_STATS, {
        "unknown linkage": dict(kind=2), "negative linkage": dict(kind=-1), "valid average": dict(kind=capi.LINKAGE_AVERAGE),
        "valid one row, NULL merges": dict(row_begin=9, row_end=10, merges=False)}),
    "snn": merged(NULL_GRAPH, LISTS_FRONT, VALID_K, {"unknown flags": dict(flags=2), "all flags": dict(flags=0xFFFFFFFF), "valid closed": dict(flags=capi.SNN_CLOSED)}),
    "jarvis_patrick": merged(nulls("db", "cluster_of", "nclusters"), LISTS_FRONT, NO_STATS, {
        "unknown flags": dict(flags=4), "all flags": dict(flags=0xFFFFFFFF), "NULL kmins": dict(kmins=None), "no levels": dict(nlevels=0),
        "nine levels": dict(kmins=tuple(range(9)), k=10), "a kmin above k": dict(kmins=(1, 6)),
        "a kmin above k + 2, closed": dict(kmins=(1, 8), flags=capi.SNN_CLOSED), "descending kmins": dict(kmins=(2, 1)), "equal kmins": dict(kmins=(2, 2)),
        "valid kmin k + 2, closed": dict(kmins=(1, 7), flags=capi.SNN_CLOSED), "valid either": dict(flags=capi.SNN_EITHER),
        "valid eight levels": dict(kmins=tuple(range(8)), k=10), "valid one level": dict(kmins=(0,)), "valid k 1": dict(k=1, kmins=(0, 1)),
        "valid k largest": dict(k=capi.KNN_MAX_K),
        "valid outputs not asked for": dict(first_row=False, sizes=False)}),
}
EMPTY = {"label_sums": dict(labels=()), "labelset_create": dict(labels=())}
CSR = single.CSR
SCORED = {"NULL scores": dict(scores=None), "a NaN score": dict(scores=(0.5, 0.5, nan, 0.75, 0.25, 0.25)),
          "valid no edges, NULL scores": dict(indptr=(0,) * 8, indices=None, scores=None), "min_pts 0": dict(min_pts=0),
          "valid min_pts 1": dict(min_pts=1), "valid min_pts 3": dict(min_pts=3), "valid min_pts huge": dict(min_pts=0xFFFFFFFF)}
GRAPH_ENTRIES = {
    "dbscan": merged(CSR, SCORED, nulls("label_of", "nclusters"), {"valid outputs not asked for": dict(anchor=False, first_row=False, sizes=False)}),
    "mreach_mst": merged(CSR, SCORED, nulls("edges", "nedges"), {
        "valid without core": dict(core=False), "valid one row, NULL edges": dict(indptr=(0, 0), indices=None, scores=None, nrows=1, edges=False)}),
    "mst_hdbscan": merged(nulls("label_of", "nclusters"), SELECTION, {
        "NULL edges": dict(edges=None, nedges=3), "2^32 rows": dict(edges=(), nrows=1 << 32), "an edge with a == b": dict(edges=((1, 1, 0.5),)),
        "an edge with a > b": dict(edges=((2, 1, 0.5),)), "an edge to nrows": dict(edges=((1, 7, 0.5),)), "a NaN edge score": dict(edges=((1, 2, nan),)),
        "as many edges as rows": dict(edges=((0, 1, 0.5), (0, 1, 0.5)), nrows=2), "a NaN floor": dict(floor=nan),
        "ascending edge scores": dict(edges=((0, 1, 0.5), (1, 2, 0.75))), "a floor above an edge": dict(floor=0.5),
        "a cycle": dict(edges=((0, 1, 0.75), (1, 2, 0.75), (0, 2, 0.5))), "valid": dict(), "valid floor 0": dict(floor=0.0),
        "valid min_cluster_size 3": dict(min_cluster_size=3), "valid no edges": dict(edges=()), "valid no rows": dict(edges=(), nrows=0),
        "valid NULL edges with nedges 0": dict(edges=None, nedges=0), "valid without roots": dict(flags=capi.HDBSCAN_NO_ROOTS),
        "valid outputs not asked for": dict(leave=False, first_row=False, sizes=False, birth=False, stability=False)}),
    "linkage": merged(nulls("merges", "nmerges"), {
        "NULL scores": dict(scores=None, n=4), "more than 65536 rows": dict(scores=None, n=capi.LINKAGE_MAX_ROWS + 1, ld=capi.LINKAGE_MAX_ROWS + 1), "unknown linkage": dict(kind=2),
        "negative linkage": dict(kind=-1), "ld below n": dict(ld=3), "a NaN score": dict(scores=((1.0, nan), (nan, 1.0))),
        "a score above 1": dict(scores=((1.0, 1.5), (1.5, 1.0))), "a negative score": dict(scores=((1.0, -0.5), (-0.5, 1.0))),
        "valid": dict(), "valid average": dict(kind=capi.LINKAGE_AVERAGE), "valid without scans": dict(scans=False),
        "valid a NaN below the diagonal": dict(scores=((1.0, 0.5), (nan, 1.0))), "valid one row, NULL scores and merges": dict(scores=None, n=1, merges=False),
        "valid no rows": dict(scores=None, n=0, merges=False)}),
    "snn": merged(CSR, nulls("shared"), {
        "unknown flags": dict(flags=2), "all flags": dict(flags=0xFFFFFFFF), "a list with its own row": dict(indices=(1, 2, 0, 2, 0, 1, 0, 4, 4)),
        "a list with a row twice": dict(indices=(1, 1, 0, 2, 0, 1, 0, 4, 3)), "valid closed": dict(flags=capi.SNN_CLOSED),
        "valid no edges, NULL shared": dict(indptr=(0,) * 8, indices=None, shared=False)}),
    "jarvis_patrick": merged(CSR, nulls("cluster_of", "nclusters"), {
        "NULL kmins": dict(kmins=None), "unknown flags": dict(flags=4), "all flags": dict(flags=0xFFFFFFFF), "no levels": dict(nlevels=0),
        "nine levels": dict(kmins=tuple(range(9))), "descending kmins": dict(kmins=(2, 1)), "equal kmins": dict(kmins=(1, 1)),
        "a list with its own row": dict(indices=(1, 2, 0, 2, 0, 1, 0, 4, 4)), "a list with a row twice": dict(indices=(1, 1, 0, 2, 0, 1, 0, 4, 3)),
        "valid closed": dict(flags=capi.SNN_CLOSED), "valid either": dict(flags=capi.SNN_EITHER), "valid one level": dict(kmins=(1,)),
        "valid eight levels": dict(kmins=tuple(range(8))), "valid outputs not asked for": dict(first_row=False, sizes=False)}),
}
# the graph cases of the CSR table that name GRAPH's arrays, on the lists
LISTS_CSR = {"indptr[0] != 0": dict(indptr=(1, 2, 4, 6, 8, 9, 9, 9)), "a decreasing indptr": dict(indptr=(0, 2, 4, 3, 8, 9, 9, 9)),
             "a column index equal to nrows": dict(indices=(1, 2, 0, 2, 0, 1, 0, 7, 3))}


def run_all():
    L = capi.load()
    got = {}

    def record(case, result):
        code, out = result
        got[case] = {"code": int(code), "message": L.gsim_last_error().decode() if code != 0 else "", "out": out}

    t = Calls()
    for entry, cases in ENTRIES.items():
        for what, kw in cases.items():
            record("%s: %s" % (entry, what), getattr(t, entry)(**kw))
    t.close()
    # rows one word too wide and of the widest width, no rows at all, one row, and more rows than a dendrogram takes
    wide, widest, empty, one = Calls(bits=4128, rows=3), Calls(bits=4096, rows=3), Calls(rows=0), Calls(rows=1)
    for entry in ENTRIES:
        record("%s: 4128-bit rows" % entry, getattr(wide, entry)())
        record("%s: valid 4096-bit rows" % entry, getattr(widest, entry)())
        record("%s: valid empty table" % entry, getattr(empty, entry)(**EMPTY.get(entry, {})))
        record("%s: valid table of one row" % entry, getattr(one, entry)())
    for entry in ("core_scores", "hdbscan", "jarvis_patrick"):
        record("%s: valid empty table, NULL row outputs" % entry, getattr(empty, entry)(**{{"core_scores": "core", "hdbscan": "label_of",
                                                                                             "jarvis_patrick": "cluster_of"}[entry]: False}))
    record("mreach_mst: valid table of one row, NULL edges", one.mreach_mst(edges=False))
    for x in (wide, widest, empty, one):
        x.close()
    long = Calls(bits=32, rows=capi.LINKAGE_MAX_ROWS + 1)
    record("linkage: more than 65536 rows", long.linkage())
    record("linkage: valid 65536 rows of a longer table", long.linkage(row_begin=1))
    long.close()
    g = Graphs()
    for entry, cases in GRAPH_ENTRIES.items():
        for what, kw in cases.items():
            if entry in ("snn", "jarvis_patrick") and what in LISTS_CSR:
                kw = LISTS_CSR[what]
            record("gsim_%s: %s" % (entry, what), getattr(g, entry)(**kw))
    return got
