"""The case list that scripts/make_front_errors_golden.py records and tests/test_front_errors_host.py replays: every front of the
two-table calls, and gsim_db_knn, on tables that are not on a GPU -- one argument changed at a time from a valid call, and a handful
of valid calls (a state error: the tables have no rows on a GPU).  `run_all()` returns {case id: {code, message, out_cleared}};
out_cleared is None for an entry without `out`, or when NULL was passed for it."""
import ctypes as C

import numpy as np

from gpusimilarity_amd import capi

TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
inf, nan = float("inf"), float("nan")
F = np.float32
FP, U32P, U64P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
GARBAGE = 0xDEAD0
EDGES = (0.25, 0.5, 0.75, 1.0)
ROWS, LROWS, NQ = 40, 30, 7
HUGE = dict(lrow_begin=1 << 40, lrow_end=(1 << 40) + (1 << 33))


def host_table(bits, rows):
    W = bits // 32
    return capi.Table(bits).add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))


class Tables:
    """A table, a second handle of the same width (`left`: "other"), the table itself ("same") or none (None), and host queries."""

    def __init__(self, bits=1024, rows=ROWS, lrows=LROWS, lbits=None):
        self.t = host_table(bits, rows)
        self.left = host_table(lbits or bits, lrows)
        self.q = np.ones((NQ, bits // 32), np.uint32)
        self.rows, self.lrows = rows, lrows
        self.keep = []

    def close(self):
        self.t.close()
        self.left.close()

    def handles(self, db, left, lrow_end):
        lh = {"other": self.left._h, "same": self.t._h, None: None}[left]
        if lrow_end is None:
            lrow_end = self.rows if left == "same" else self.lrows if left == "other" else 0
        return self.t._h if db else None, lh, lrow_end

    def queries(self, queries):
        return self.q.ctypes.data_as(U32P) if queries else None

    def edges(self, edges, nedges):
        e = np.asarray(edges if edges is not None else [], F)
        self.keep = [e, np.zeros((64, len(e) + 1), np.uint64), np.zeros(len(e) + 1, np.uint64), np.zeros(64 * 64, F)]
        return e.ctypes.data_as(FP) if edges is not None else None, len(e) if nedges is None else nedges

    def graph(self, fn, out):
        """A graph-returning call: `*out` holds garbage before it."""
        g = C.c_void_p(GARBAGE)
        code = fn(C.byref(g) if out else None)
        return code, (g.value is None) if out else None

    # -- the ten entry points, every argument with a valid default --
    def join(self, db=True, left="other", lrow_begin=0, lrow_end=None, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, order=0, out=True):
        d, lh, le = self.handles(db, left, lrow_end)
        return self.graph(lambda o: capi.load().gsim_db_join(d, lh, lrow_begin, le, cutoff, metric, alpha, beta, order, o), out)

    def join_queries(self, db=True, queries=True, nq=NQ, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, order=0, out=True):
        return self.graph(lambda o: capi.load().gsim_db_join_queries(self.t._h if db else None, self.queries(queries), nq, cutoff, metric,
                                                                     alpha, beta, order, o), out)

    def knn_join(self, db=True, left="other", lrow_begin=0, lrow_end=None, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, flags=0,
                 out=True):
        d, lh, le = self.handles(db, left, lrow_end)
        return self.graph(lambda o: capi.load().gsim_db_knn_join(d, lh, lrow_begin, le, k, cutoff, metric, alpha, beta, flags, o), out)

    def knn_queries(self, db=True, queries=True, nq=NQ, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, out=True):
        return self.graph(lambda o: capi.load().gsim_db_knn_queries(self.t._h if db else None, self.queries(queries), nq, k, cutoff, metric,
                                                                    alpha, beta, o), out)

    def knn(self, db=True, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, row_begin=0, row_end=ROWS, out=True):
        return self.graph(lambda o: capi.load().gsim_db_knn(self.t._h if db else None, k, cutoff, metric, alpha, beta, row_begin, row_end, o),
                          out)

    def histogram(self, db=True, left="other", lrow_begin=0, lrow_end=None, edges=EDGES, nedges=None, metric=TAN, alpha=1.0, beta=1.0,
                  flags=0, hist=True, total=True):
        d, lh, le = self.handles(db, left, lrow_end)
        ep, n = self.edges(edges, nedges)
        hp, tp = (self.keep[1].ctypes.data_as(U64P) if hist else None), (self.keep[2].ctypes.data_as(U64P) if total else None)
        return capi.load().gsim_db_histogram(d, lh, lrow_begin, le, ep, n, metric, alpha, beta, flags, hp, tp, None), None

    def histogram_queries(self, db=True, queries=True, nq=NQ, edges=EDGES, nedges=None, metric=TAN, alpha=1.0, beta=1.0, hist=True,
                          total=True):
        ep, n = self.edges(edges, nedges)
        hp, tp = (self.keep[1].ctypes.data_as(U64P) if hist else None), (self.keep[2].ctypes.data_as(U64P) if total else None)
        return capi.load().gsim_db_histogram_queries(self.t._h if db else None, self.queries(queries), nq, ep, n, metric, alpha, beta, hp, tp,
                                                     None), None

    def scores(self, entry="gsim_db_scores", db=True, left="other", lrow_begin=0, lrow_end=None, col_begin=0, col_end=None, metric=TAN,
               alpha=1.0, beta=1.0, out=True, ld=None):
        d, lh, le = self.handles(db, left, lrow_end)
        col_end = self.rows if col_end is None else col_end
        ld = max(col_end - col_begin, 0) if ld is None else ld
        self.edges((), None)
        o = self.keep[3].ctypes.data_as(FP) if out else None
        if entry == "gsim_db_scores_device":
            o = C.cast(o, C.c_void_p)
        return getattr(capi.load(), entry)(d, lh, lrow_begin, le, col_begin, col_end, metric, alpha, beta, o, ld, None), None

    def scores_device(self, **kw):
        return self.scores(entry="gsim_db_scores_device", **kw)

    def scores_queries(self, db=True, queries=True, nq=NQ, col_begin=0, col_end=None, metric=TAN, alpha=1.0, beta=1.0, out=True, ld=None):
        col_end = self.rows if col_end is None else col_end
        ld = max(col_end - col_begin, 0) if ld is None else ld
        self.edges((), None)
        return capi.load().gsim_db_scores_queries(self.t._h if db else None, self.queries(queries), nq, col_begin, col_end, metric, alpha, beta,
                                                  self.keep[3].ctypes.data_as(FP) if out else None, ld, None), None


METRIC = {
    "unknown metric": dict(metric=7), "negative metric": dict(metric=-1), "metric 2": dict(metric=2),
    "negative alpha": dict(metric=TV, alpha=-0.5, beta=0.5), "negative beta": dict(metric=TV, alpha=0.5, beta=-0.5),
    "infinite alpha": dict(metric=TV, alpha=inf, beta=0.5), "infinite beta": dict(metric=TV, alpha=0.5, beta=inf),
    "-infinite alpha": dict(metric=TV, alpha=-inf, beta=1.0), "NaN alpha": dict(metric=TV, alpha=nan, beta=0.5),
    "NaN beta": dict(metric=TV, alpha=0.5, beta=nan),
}
VALID_METRIC = {
    "valid": dict(), "valid Tversky .5 .5": dict(metric=TV, alpha=0.5, beta=0.5), "valid Tversky .3 .7": dict(metric=TV, alpha=0.3, beta=0.7),
    "valid Tversky 1 0": dict(metric=TV, alpha=1.0, beta=0.0), "valid Tversky 0 0": dict(metric=TV, alpha=0.0, beta=0.0),
    "valid Tanimoto ignores alpha and beta": dict(metric=TAN, alpha=-1.0, beta=nan),
}
CUTOFF = {"cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff 1.5": dict(cutoff=1.5),
          "cutoff NaN": dict(cutoff=nan), "cutoff inf": dict(cutoff=inf)}
VALID_CUTOFF = {"valid cutoff 1": dict(cutoff=1.0), "valid cutoff tiny": dict(cutoff=float(np.nextafter(F(0), F(1))))}
K = {"k 0": dict(k=0), "k above the largest": dict(k=capi.KNN_MAX_K + 1), "k huge": dict(k=0xFFFFFFFF)}
VALID_K = {"valid k 1": dict(k=1), "valid k largest": dict(k=capi.KNN_MAX_K)}
ORDER = {"order 2": dict(order=2), "order -1": dict(order=-1)}
NULL_GRAPH = {"NULL db": dict(db=False), "NULL out": dict(out=False)}
LEFT = {  # the handle fronts
    "NULL left": dict(left=None), "lrow_begin > lrow_end": dict(lrow_begin=7, lrow_end=6), "lrow_end past the left count": dict(lrow_end=LROWS + 1),
    "both past the left count": dict(lrow_begin=LROWS + 1, lrow_end=LROWS + 1),
    "lrow_end past the count, left == db": dict(left="same", lrow_end=ROWS + 1),
    "a range of the table's size on a shorter left table": dict(lrow_end=ROWS), "a huge range far past the left table": HUGE,
    "a huge range, left == db": dict(left="same", **HUGE),
}
VALID_LEFT = {
    "valid left == db": dict(left="same"), "valid range": dict(lrow_begin=3, lrow_end=17), "valid empty range": dict(lrow_begin=9, lrow_end=9),
    "valid empty range at the end": dict(lrow_begin=LROWS, lrow_end=LROWS), "valid range, left == db": dict(left="same", lrow_begin=5, lrow_end=ROWS),
}
QUERIES = {"NULL queries with nq > 0": dict(queries=False), "nq 2^32": dict(nq=1 << 32)}
VALID_QUERIES = {"valid nq 1": dict(nq=1), "valid nq 0": dict(nq=0), "valid NULL queries with nq 0": dict(queries=False, nq=0),
                 "valid nq 2^32 - 1": dict(nq=(1 << 32) - 1)}
FLAGS = {  # knn join (GSIM_KNN_EXCLUDE_SELF) and histogram (GSIM_HIST_EXCLUDE_SELF): both are bit 0
    "unknown flag bits": dict(flags=2), "unknown flag bits beside the known one": dict(left="same", flags=3),
    "the top flag bit beside the known one": dict(left="same", flags=0x80000001), "all flag bits": dict(flags=0xFFFFFFFF),
    "the self flag with left != db": dict(flags=1),
}
VALID_FLAGS = {"valid self flag": dict(left="same", flags=1), "valid self flag on a range": dict(left="same", lrow_begin=5, lrow_end=ROWS, flags=1)}
HIST = {
    "NULL edges": dict(edges=None, nedges=4), "no edges": dict(edges=(), nedges=0), "nedges 0 with edges": dict(nedges=0),
    "129 edges": dict(edges=tuple((k + 1) / 130 for k in range(129))),
    "a descending pair": dict(edges=(0.25, 0.75, 0.5, 1.0)), "an equal pair": dict(edges=(0.25, 0.5, 0.5, 1.0)),
    "a NaN edge": dict(edges=(0.25, nan, 0.75)), "a NaN first edge": dict(edges=(nan, 0.5)), "an infinite edge": dict(edges=(0.25, 0.5, inf)),
    "edges[0] == 0": dict(edges=(0.0, 0.5)), "edges[0] < 0": dict(edges=(-0.25, 0.5)), "edges[0] == -0.0": dict(edges=(-0.0, 0.5)),
    "both outputs NULL": dict(hist=False, total=False), "NULL db": dict(db=False),
}
VALID_HIST = {
    "valid one edge": dict(edges=(0.5,)), "valid 128 edges": dict(edges=tuple((k + 1) / 129 for k in range(128))),
    "valid edges above 1": dict(edges=(0.5, 1.0, 1.5)), "valid tiny edge": dict(edges=(float(np.nextafter(F(0), F(1))),)),
    "valid without hist": dict(hist=False), "valid without total": dict(total=False),
}
SCORES = {
    "NULL db": dict(db=False), "NULL out": dict(out=False), "ld < nr": dict(ld=ROWS - 1), "ld < nr of a range": dict(col_begin=10, col_end=30, ld=19),
    "ld 0": dict(ld=0), "col_begin > col_end": dict(col_begin=7, col_end=6, ld=ROWS), "col_end past the count": dict(col_end=ROWS + 1, ld=ROWS + 1),
}
VALID_SCORES = {
    "valid ld": dict(ld=ROWS), "valid wide ld": dict(ld=1000), "valid columns": dict(col_begin=5, col_end=17), "valid columns, wide ld": dict(col_begin=5, col_end=17, ld=64),
    "valid no columns": dict(col_begin=9, col_end=9), "valid no columns, NULL out": dict(col_begin=9, col_end=9, out=False),
}
KNN_RANGE = {"row_begin > row_end": dict(row_begin=7, row_end=6), "row_end past the count": dict(row_end=ROWS + 1),
             "both past the count": dict(row_begin=ROWS + 1, row_end=ROWS + 1)}
VALID_KNN_RANGE = {"valid range": dict(row_begin=3, row_end=17), "valid empty range": dict(row_begin=9, row_end=9)}


def merged(*groups):
    out = {}
    for g in groups:
        for what, kw in g.items():
            assert what not in out, what
            out[what] = kw
    return out


GRAPH_HANDLE = merged(NULL_GRAPH, METRIC, VALID_METRIC, CUTOFF, VALID_CUTOFF, LEFT, VALID_LEFT)
GRAPH_QUERIES = merged(NULL_GRAPH, METRIC, VALID_METRIC, CUTOFF, VALID_CUTOFF, QUERIES, VALID_QUERIES)
ENTRIES = {
    "join": merged(GRAPH_HANDLE, ORDER, {"valid by score": dict(order=capi.JOIN_BY_SCORE)}),
    "join_queries": merged(GRAPH_QUERIES, ORDER, {"valid by score": dict(order=capi.JOIN_BY_SCORE)}),
    "knn_join": merged(GRAPH_HANDLE, K, VALID_K, FLAGS, VALID_FLAGS),
    "knn_queries": merged(GRAPH_QUERIES, K, VALID_K),
    "knn": merged(NULL_GRAPH, METRIC, VALID_METRIC, CUTOFF, VALID_CUTOFF, K, VALID_K, KNN_RANGE, VALID_KNN_RANGE),
    "histogram": merged(HIST, VALID_HIST, METRIC, VALID_METRIC, LEFT, VALID_LEFT, FLAGS, VALID_FLAGS),
    "histogram_queries": merged(HIST, VALID_HIST, METRIC, VALID_METRIC, QUERIES, VALID_QUERIES),
    "scores": merged(SCORES, VALID_SCORES, METRIC, VALID_METRIC, LEFT, VALID_LEFT),
    "scores_device": merged(SCORES, VALID_SCORES, METRIC, VALID_METRIC, LEFT, VALID_LEFT),
    "scores_queries": merged(SCORES, VALID_SCORES, METRIC, VALID_METRIC, QUERIES, VALID_QUERIES),
}
HANDLE_FRONTS = ("join", "knn_join", "histogram", "scores", "scores_device")


def run_all():
    L = capi.load()
    got = {}

    def record(case, result):
        code, cleared = result
        got[case] = {"code": int(code), "message": L.gsim_last_error().decode() if code != 0 else "", "out_cleared": cleared}

    t = Tables()
    for entry, cases in ENTRIES.items():
        for what, kw in cases.items():
            record("%s: %s" % (entry, what), getattr(t, entry)(**kw))
    t.close()
    # unequal fp_bits (the handle fronts), rows of 4128 bits (one word too wide) and of 4096 (the widest)
    mixed, wide, widest = Tables(lbits=512), Tables(bits=4128, rows=3, lrows=3), Tables(bits=4096, rows=3, lrows=3)
    for entry in ENTRIES:
        kw = dict(row_end=3) if entry == "knn" else {}
        if entry in HANDLE_FRONTS:
            record("%s: unequal fp_bits" % entry, getattr(mixed, entry)())
        record("%s: 4128-bit rows" % entry, getattr(wide, entry)(**kw))
        record("%s: valid 4096-bit rows" % entry, getattr(widest, entry)(**kw))
    for x in (mixed, wide, widest):
        x.close()
    return got
