"""The case list of the single-table fronts and the host functions on a caller's CSR graph, recorded by
scripts/make_front_errors_golden.py (list "single") and replayed by tests/test_single_front_errors_host.py: the fifteen entry points
that work on one table, on tables that are not on a GPU -- one argument changed at a time from a valid call, and a handful of valid
calls (a state error: the tables have no rows on a GPU; GSIM_OK on an empty table where the call answers without one) -- and
gsim_butina, gsim_components, gsim_mst and gsim_mst_cut on host arrays.  `run_all()` returns {case id: {code, message, out}}; `out`
names every output of the call: "untouched" (it still holds what was there before the call), the values it holds now, or None
where NULL was passed for it.

A row set cannot be made without a GPU.  Where a front reads one before any device state, the cases pass a stand-in: zeroed
memory that begins as gsim_rowset does (capi_internal.h), with the owner and the row count the case asks for."""
import ctypes as C

import numpy as np

from front_errors_cases import (CUTOFF, GARBAGE, K, KNN_RANGE, METRIC, NULL_GRAPH, VALID_CUTOFF, VALID_K, VALID_KNN_RANGE, VALID_METRIC,
                                host_table, merged)
from gpusimilarity_amd import capi

TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
inf, nan = float("inf"), float("nan")
FP, U32P, U64P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
ROWS = 40
FILL = 0xA5  # every byte of an output before the call


class FakeRowset(C.Structure):
    _fields_ = [("owner", C.c_void_p), ("device", C.c_int), ("nrows", C.c_uint64), ("count", C.c_uint64), ("row_base", C.c_uint32),
                ("rest", C.c_uint8 * 256)]


class Calls:
    """One host table and the entry points on it, every argument with a valid default.  An output is a named array or struct full
    of FILL bytes; False passes NULL for it.  `table`: a capi.Table of that shape to call instead (tests/test_gpu_single_front_states.py)."""

    def __init__(self, bits=1024, rows=ROWS, table=None):
        self.t = table or host_table(bits, rows)
        self.other = host_table(bits, 3)
        self.rows, self.W, self.bits = rows, bits // 32, bits
        self.outs, self.keep = {}, []

    def close(self):
        self.t.close()
        self.other.close()

    # -- arguments --
    def db(self, db):
        return self.t._h if db else None

    def inp(self, values, dtype, ptr):
        """An input array, or NULL for None"""
        if values is None:
            return None
        a = np.ascontiguousarray(values, dtype)
        self.keep.append(a)
        return a.ctypes.data_as(ptr) if ptr is not None else a.ctypes.data

    def out(self, name, give, nbytes, ptr=U32P):
        if not give:
            self.outs[name] = None
            return None
        a = np.full(max(nbytes, 4), FILL, np.uint8)
        self.outs[name] = a
        return a.ctypes.data_as(ptr) if ptr is not None else a.ctypes.data

    def stats(self, cls, give=True):
        if not give:
            self.outs["stats"] = None
            return None
        s = cls()
        C.memset(C.byref(s), FILL, C.sizeof(s))
        self.outs["stats"] = s
        return C.byref(s)

    def rowset(self, rs):
        """None, or a stand-in row set: "mine" (owner: the table), "other" (another handle), "stale" (the table, another row count)"""
        if rs is None:
            return None
        f = FakeRowset()
        f.owner = (self.other if rs == "other" else self.t)._h.value
        f.nrows = self.rows + (5 if rs == "stale" else 0)
        self.keep.append(f)
        return C.cast(C.byref(f), C.c_void_p)

    def seen(self, code):
        got = {}
        for name, o in self.outs.items():
            if o is None:
                got[name] = None
                continue
            raw = np.frombuffer(bytes(o), np.uint8) if isinstance(o, C.Structure) else o
            if (raw == FILL).all():
                got[name] = "untouched"
            elif not raw.any():
                got[name] = "zero"
            else:
                got[name] = raw[:len(raw) // 4 * 4].view(np.uint32).tolist()
        self.outs, self.keep = {}, []
        return code, got

    def graph(self, fn, out):
        g = C.c_void_p(GARBAGE)
        code = fn(C.byref(g) if out else None)
        return code, {"out": ("cleared" if g.value is None else "untouched") if out else None}

    # -- the fifteen entry points --
    def neighbors(self, db=True, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, row_begin=0, row_end=None, out=True):
        re = self.rows if row_end is None else row_end
        return self.graph(lambda o: capi.load().gsim_db_neighbors(self.db(db), cutoff, metric, alpha, beta, row_begin, re, o), out)

    def knn(self, db=True, k=5, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, row_begin=0, row_end=None, out=True):
        re = self.rows if row_end is None else row_end
        return self.graph(lambda o: capi.load().gsim_db_knn(self.db(db), k, cutoff, metric, alpha, beta, row_begin, re, o), out)

    def maxmin(self, db=True, npicks=5, seeds=(3, 9), nseeds=None, metric=TAN, alpha=1.0, beta=1.0, max_score=1.0, picks=True, npicked=True,
               stats=True):
        ns = (len(seeds) if seeds is not None else 0) if nseeds is None else nseeds
        return self.seen(capi.load().gsim_db_maxmin(
            self.db(db), npicks, self.inp(seeds, np.uint32, U32P), ns, metric, alpha, beta, max_score, self.out("picks", picks, 4 * max(npicks, 1)),
            self.out("pick_scores", True, 4 * max(npicks, 1), FP), self.out("npicked", npicked, 4), self.out("row_score", True, 4 * self.rows, FP),
            self.out("nearest", True, 4 * self.rows), self.stats(capi.GsimMaxMinStats, stats)))

    def leader(self, db=True, cutoff=0.5, seeds=(3, 9), nseeds=None, max_leaders=10, metric=TAN, alpha=1.0, beta=1.0, leaders=True, nleaders=True,
               stats=True):
        ns = (len(seeds) if seeds is not None else 0) if nseeds is None else nseeds
        return self.seen(capi.load().gsim_db_leader(
            self.db(db), cutoff, self.inp(seeds, np.uint32, U32P), ns, max_leaders, metric, alpha, beta, self.out("leaders", leaders, 4 * ROWS),
            self.out("nleaders", nleaders, 4), self.out("leader_of", True, 4 * self.rows), self.out("row_score", True, 4 * self.rows, FP),
            self.stats(capi.GsimLeaderStats, stats)))

    def components(self, db=True, cutoffs=(0.3, 0.5, 0.7), nlevels=None, metric=TAN, alpha=1.0, beta=1.0, component_of=True, ncomponents=True,
                   stats=True):
        nl = (len(cutoffs) if cutoffs is not None else 1) if nlevels is None else nlevels
        return self.seen(capi.load().gsim_db_components(
            self.db(db), self.inp(cutoffs, np.float32, FP), nl, metric, alpha, beta, self.out("component_of", component_of, 4 * 8 * self.rows),
            self.out("ncomponents", ncomponents, 4 * 8), self.out("first_row", True, 4 * 8 * self.rows), self.out("sizes", True, 4 * 8 * self.rows),
            self.stats(capi.GsimComponentsStats, stats)))

    def mst(self, db=True, cutoff=0.5, metric=TAN, alpha=1.0, beta=1.0, edges=True, nedges=True, stats=True):
        return self.seen(capi.load().gsim_db_mst(self.db(db), cutoff, metric, alpha, beta, self.out("edges", edges, 12 * self.rows, None),
                                                 self.out("nedges", nedges, 8, U64P), self.stats(capi.GsimMstStats, stats)))

    def bit_counts(self, db=True, rs=None, row_begin=0, row_end=None, counts=True, counted=True, stats=True):
        re = self.rows if row_end is None else row_end
        return self.seen(capi.load().gsim_db_bit_counts(self.db(db), self.rowset(rs), row_begin, re, self.out("counts", counts, 8 * self.bits, U64P),
                                                        self.out("counted", counted, 8, U64P), self.stats(capi.GsimProfileStats, stats)))

    def overlap_sums(self, db=True, weights=True, row_begin=0, row_end=None, sums=True, stats=True):
        re = self.rows if row_end is None else row_end
        w = self.inp(np.ones(self.bits), np.uint32, U32P) if weights else None
        return self.seen(capi.load().gsim_db_overlap_sums(self.db(db), w, row_begin, re, self.out("sums", sums, 8 * self.rows, U64P),
                                                          self.out("popc", True, 4 * self.rows), self.stats(capi.GsimProfileStats, stats)))

    def assign(self, db=True, centres=True, m=3, row_begin=0, row_end=None, metric=TAN, alpha=1.0, beta=1.0, label=True, stats=True):
        re = self.rows if row_end is None else row_end
        c = self.inp(np.ones((3, self.W)), np.uint32, U32P) if centres else None
        return self.seen(capi.load().gsim_db_assign(self.db(db), c, m, row_begin, re, metric, alpha, beta, self.out("label", label, 4 * self.rows),
                                                    self.out("score", True, 4 * self.rows, FP), self.stats(capi.GsimAssignStats, stats)))

    def label_counts(self, db=True, labels="fit", nlabels=3, row_begin=0, row_end=None, counts=True, sizes=True, stats=True):
        re = self.rows if row_end is None else row_end
        lab = np.arange(max(re - row_begin, 0) if re <= 10 * ROWS else 0) % 3 if isinstance(labels, str) else labels
        return self.seen(capi.load().gsim_db_label_counts(
            self.db(db), self.inp(lab, np.uint32, U32P), nlabels, row_begin, re, self.out("counts", counts, 4 * 3 * self.bits),
            self.out("sizes", sizes, 4 * 3), self.stats(capi.GsimLabelStats, stats)))

    def kmeans(self, db=True, init=True, m=3, max_iter=4, metric=TAN, alpha=1.0, beta=1.0, centres=True, label=True, stats=True):
        i = self.inp(np.ones((3, self.W)), np.uint32, U32P) if init else None
        return self.seen(capi.load().gsim_db_kmeans(
            self.db(db), i, m, max_iter, metric, alpha, beta, self.out("centres", centres, 4 * 3 * self.W), self.out("label", label, 4 * self.rows),
            self.out("score", True, 4 * self.rows, FP), self.out("sizes", True, 4 * 3), self.stats(capi.GsimKmeansStats, stats)))

    def search_group(self, db=True, queries=True, nq=4, mode=capi.GROUP_MAX, k=5, cutoff=0.0, metric=TAN, alpha=1.0, beta=1.0, hits=True, count=True,
                     stats=True):
        q = self.inp(np.ones((4, self.W)), np.uint32, U32P) if queries else None
        return self.seen(capi.load().gsim_db_search_group(self.db(db), q, nq, mode, k, cutoff, metric, alpha, beta, self.out("hits", hits, 12 * 5, None),
                                                          self.out("count", count, 4), self.out("approx", True, 8, U64P),
                                                          self.stats(capi.GsimGroupStats, stats)))

    def rowset_from_rows(self, db=True, rows=(1, 5, 8), n=None, flags=0, out=True):
        r = self.inp(rows, np.uint32, U32P)
        n = (len(rows) if rows is not None else 0) if n is None else n
        return self.graph(lambda o: capi.load().gsim_rowset_from_rows(self.db(db), r, n, flags, o), out)

    def rowset_from_bitmap(self, db=True, bits=True, flags=0, out=True):
        b = self.inp(np.ones((self.rows + 31) // 32), np.uint32, U32P) if bits else None
        return self.graph(lambda o: capi.load().gsim_rowset_from_bitmap(self.db(db), b, flags, o), out)

    def search_rows(self, db=True, rs="mine", queries=True, nq=2, k=5, cutoff=0.0, metric=TAN, alpha=1.0, beta=1.0, hits=True, counts=True, stats=True):
        q = self.inp(np.ones((2, self.W)), np.uint32, U32P) if queries else None
        return self.seen(capi.load().gsim_db_search_rows(self.db(db), self.rowset(rs), q, nq, k, cutoff, metric, alpha, beta,
                                                         self.out("hits", hits, 12 * 2 * 5, None), self.out("counts", counts, 4 * 2),
                                                         self.out("approx", True, 8 * 2, U64P), self.stats(capi.GsimRowsetStats, stats)))


# ---- the host functions on a caller's graph: a path 0-1-2, the pair 4-5 and the lone rows 3 and 6, every edge listed both ways ----
GRAPH = dict(indptr=(0, 1, 3, 4, 4, 5, 6, 6), indices=(1, 0, 2, 1, 5, 4), scores=(0.5, 0.5, 0.75, 0.75, 0.25, 0.25), nrows=7)
CUT_EDGES = ((1, 2, 0.75), (0, 1, 0.5), (4, 5, 0.25))


class Graphs(Calls):
    def __init__(self):
        self.outs, self.keep = {}, []

    def close(self):
        pass

    def csr(self, indptr, indices, scores=None):
        return self.inp(indptr, np.uint64, U64P), self.inp(indices, np.uint32, U32P), self.inp(scores, np.float32, FP)

    def butina(self, indptr=GRAPH["indptr"], indices=GRAPH["indices"], nrows=GRAPH["nrows"], cluster_of=True, centroids=True, nclusters=True):
        ip, ix, _ = self.csr(indptr, indices)
        return self.seen(capi.load().gsim_butina(ip, ix, nrows, self.out("cluster_of", cluster_of, 4 * 7), self.out("centroids", centroids, 4 * 7),
                                                 self.out("nclusters", nclusters, 8, U64P)))

    def components(self, indptr=GRAPH["indptr"], indices=GRAPH["indices"], nrows=GRAPH["nrows"], component_of=True, first_row=True, sizes=True,
                   ncomponents=True):
        ip, ix, _ = self.csr(indptr, indices)
        return self.seen(capi.load().gsim_components(ip, ix, nrows, self.out("component_of", component_of, 4 * 7), self.out("first_row", first_row, 4 * 7),
                                                     self.out("sizes", sizes, 4 * 7), self.out("ncomponents", ncomponents, 8, U64P)))

    def mst(self, indptr=GRAPH["indptr"], indices=GRAPH["indices"], scores=GRAPH["scores"], nrows=GRAPH["nrows"], edges=True, nedges=True):
        ip, ix, sc = self.csr(indptr, indices, scores)
        return self.seen(capi.load().gsim_mst(ip, ix, sc, nrows, self.out("edges", edges, 12 * 6, None), self.out("nedges", nedges, 8, U64P)))

    def mst_cut(self, edges=CUT_EDGES, nrows=GRAPH["nrows"], t=0.5, component_of=True, first_row=True, sizes=True, ncomponents=True):
        e = np.array(list(edges), capi.MST_EDGE_DTYPE)
        self.keep.append(e)
        return self.seen(capi.load().gsim_mst_cut(e.ctypes.data, len(e), nrows, t, self.out("component_of", component_of, 4 * 7),
                                                  self.out("first_row", first_row, 4 * 7), self.out("sizes", sizes, 4 * 7),
                                                  self.out("ncomponents", ncomponents, 8, U64P)))


# the symmetric calls: alpha == beta that is not finite or negative (gsim_db_neighbors alone lets them through), alpha != beta
SYMMETRIC = {
    "alpha != beta": dict(metric=TV, alpha=0.25, beta=0.75), "both infinite": dict(metric=TV, alpha=inf, beta=inf),
    "both -infinite": dict(metric=TV, alpha=-inf, beta=-inf), "both negative": dict(metric=TV, alpha=-0.5, beta=-0.5),
    "both NaN": dict(metric=TV, alpha=nan, beta=nan), "valid Tversky 2 2": dict(metric=TV, alpha=2.0, beta=2.0),
}
METRICS = merged(METRIC, VALID_METRIC, SYMMETRIC)
RANGE = {"row_begin > row_end": dict(row_begin=7, row_end=6), "row_end past the count": dict(row_end=ROWS + 1),
         "both past the count": dict(row_begin=ROWS + 1, row_end=ROWS + 1), "a huge range": dict(row_begin=1 << 40, row_end=(1 << 40) + (1 << 33)),
         "valid range": dict(row_begin=3, row_end=17), "valid empty range": dict(row_begin=9, row_end=9)}
SEEDS = {"NULL seeds": dict(seeds=None, nseeds=2), "a seed outside the table": dict(seeds=(3, ROWS)), "a huge seed": dict(seeds=(0xFFFFFFFF,)),
         "a repeated seed": dict(seeds=(3, 9, 3)), "valid no seeds": dict(seeds=()), "valid NULL seeds with nseeds 0": dict(seeds=None, nseeds=0)}


def nulls(*names):
    return {"NULL " + n: {n: False} for n in names}


ENTRIES = {
    "neighbors": merged(NULL_GRAPH, METRICS, CUTOFF, VALID_CUTOFF, KNN_RANGE, VALID_KNN_RANGE),
    "knn": merged(NULL_GRAPH, METRIC, VALID_METRIC, CUTOFF, VALID_CUTOFF, K, VALID_K, KNN_RANGE, VALID_KNN_RANGE),
    "maxmin": merged(nulls("db", "picks", "npicked"), METRICS, SEEDS, {
        "max_score < 0": dict(max_score=-0.25), "max_score > 1": dict(max_score=1.5), "max_score NaN": dict(max_score=nan),
        "more picks than rows": dict(npicks=ROWS + 1), "more seeds than picks": dict(npicks=1), "valid no picks": dict(npicks=0, seeds=()),
        "valid max_score 0": dict(max_score=0.0), "valid all rows": dict(npicks=ROWS), "valid without stats": dict(stats=False)}),
    "leader": merged(nulls("db", "leaders", "nleaders"), METRICS, CUTOFF, VALID_CUTOFF, SEEDS, {
        "max_leaders 0": dict(max_leaders=0, seeds=()), "fewer leaders than seeds": dict(max_leaders=1), "more leaders than rows": dict(max_leaders=ROWS + 1),
        "valid as many leaders as rows": dict(max_leaders=ROWS), "valid without stats": dict(stats=False)}),
    "components": merged(nulls("db", "component_of", "ncomponents"), METRICS, {
        "NULL cutoffs": dict(cutoffs=None), "no levels": dict(nlevels=0), "nine levels": dict(cutoffs=tuple((i + 1) / 10 for i in range(9))),
        "a cutoff of 0": dict(cutoffs=(0.0, 0.5)), "a cutoff above 1": dict(cutoffs=(0.5, 1.5)), "a NaN cutoff": dict(cutoffs=(0.5, nan)),
        "descending cutoffs": dict(cutoffs=(0.5, 0.3)), "equal cutoffs": dict(cutoffs=(0.5, 0.5)),
        "valid one level": dict(cutoffs=(1.0,)), "valid eight levels": dict(cutoffs=tuple((i + 1) / 8 for i in range(8))),
        "valid without stats": dict(stats=False)}),
    "mst": merged(nulls("db", "edges", "nedges"), METRICS, CUTOFF, VALID_CUTOFF, {"valid without stats": dict(stats=False)}),
    "bit_counts": merged(nulls("db", "counts"), RANGE, {
        "a row set of another handle": dict(rs="other"), "valid with a row set": dict(rs="mine"), "valid without counted": dict(counted=False),
        "valid without stats": dict(stats=False), "valid": dict()}),
    "overlap_sums": merged(nulls("db", "weights", "sums"), RANGE, {"valid NULL sums on an empty range": dict(row_begin=9, row_end=9, sums=False),
                                                                     "valid": dict()}),
    "assign": merged(nulls("db", "centres", "label"), METRIC, VALID_METRIC, RANGE, {
        "no centres": dict(m=0), "too many centres": dict(m=capi.ASSIGN_MAX_CENTRES + 1),
        "valid NULL centres and label on an empty range": dict(row_begin=9, row_end=9, centres=False, label=False), "valid without stats": dict(stats=False)}),
    "label_counts": merged(nulls("db", "counts"), RANGE, {
        "no labels": dict(nlabels=0), "NULL labels": dict(labels=None), "a label equal to nlabels": dict(labels=[0, 1, 3] + [0] * (ROWS - 3)),
        "valid unlabelled rows": dict(labels=[capi.LABEL_NONE] * ROWS), "valid NULL labels on an empty range": dict(labels=None, row_begin=9, row_end=9),
        "valid without sizes": dict(sizes=False), "valid": dict()}),
    "kmeans": merged(nulls("db", "init", "centres", "label"), METRIC, VALID_METRIC, {
        "no centres": dict(m=0), "too many centres": dict(m=capi.ASSIGN_MAX_CENTRES + 1), "max_iter 0": dict(max_iter=0),
        "valid without stats": dict(stats=False)}),
    "search_group": merged(nulls("db", "queries", "hits", "count"), METRIC, VALID_METRIC, {
        "no queries": dict(nq=0), "too many queries": dict(nq=capi.GROUP_MAX_QUERIES + 1), "unknown mode": dict(mode=3), "negative mode": dict(mode=-1),
        "Tversky alpha + beta < 1": dict(metric=TV, alpha=0.25, beta=0.25), "valid MIN": dict(mode=capi.GROUP_MIN), "valid MEAN": dict(mode=capi.GROUP_MEAN),
        "valid Tversky 1 1": dict(metric=TV, alpha=1.0, beta=1.0), "valid without stats": dict(stats=False)}),
    "rowset_from_rows": merged(NULL_GRAPH, {
        "NULL rows": dict(rows=None, n=3), "unknown flags": dict(flags=2), "all flags": dict(flags=0xFFFFFFFF), "2^32 rows given": dict(n=1 << 32),
        "a row outside the table": dict(rows=(1, ROWS)), "valid": dict(), "valid exclusion": dict(flags=1), "valid no rows": dict(rows=()),
        "valid NULL rows with n 0": dict(rows=None, n=0)}),
    "rowset_from_bitmap": merged(NULL_GRAPH, {"NULL bitmap": dict(bits=False), "unknown flags": dict(flags=2), "valid": dict(), "valid exclusion": dict(flags=1)}),
    "search_rows": merged(nulls("db", "queries", "hits", "counts"), {
        "NULL rs": dict(rs=None), "unknown metric": dict(metric=7), "negative metric": dict(metric=-1), "a row set of another handle": dict(rs="other"),
        "valid": dict(), "valid Tversky": dict(metric=TV, alpha=0.3, beta=0.7), "valid stale row set": dict(rs="stale"), "valid without stats": dict(stats=False)}),
}
# the two tables that are no 1024-bit table of 40 rows: rows one word too wide or of the widest width, and no rows at all
EMPTY = {
    "maxmin": dict(npicks=0, seeds=()), "leader": dict(seeds=()), "label_counts": dict(labels=()), "rowset_from_rows": dict(rows=()),
}
CSR = {
    "indptr[0] != 0": dict(indptr=(1, 1, 3, 4, 4, 5, 6, 6)), "a decreasing indptr": dict(indptr=(0, 1, 3, 2, 4, 5, 6, 6)),
    "NULL indices with nnz > 0": dict(indices=None), "a column index equal to nrows": dict(indices=(1, 0, 7, 1, 5, 4)),
    "2^32 rows": dict(nrows=1 << 32), "NULL indptr": dict(indptr=None), "valid": dict(),
    "valid no rows": dict(indptr=(0,), indices=None, nrows=0), "valid no edges": dict(indptr=(0,) * 8, indices=None),
}
GRAPH_ENTRIES = {
    "butina": merged(CSR, nulls("cluster_of", "centroids", "nclusters")),
    "components": merged(CSR, nulls("component_of", "ncomponents"), {"valid without first_row and sizes": dict(first_row=False, sizes=False)}),
    "mst": merged(CSR, nulls("edges", "nedges"), {"NULL scores": dict(scores=None), "a NaN score": dict(scores=(0.5, 0.5, nan, 0.75, 0.25, 0.25)),
                                                  "valid no edges, NULL scores": dict(indptr=(0,) * 8, indices=None, scores=None),
                                                  "valid one row, NULL edges": dict(indptr=(0, 0), indices=None, scores=None, nrows=1, edges=False)}),
    "mst_cut": {"valid": dict(), "valid cut above every edge": dict(t=0.9), "valid cut below every edge": dict(t=0.0),
                "valid without first_row and sizes": dict(first_row=False, sizes=False)},
}


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
    wide, widest, empty = Calls(bits=4128, rows=3), Calls(bits=4096, rows=3), Calls(rows=0)
    for entry in ENTRIES:
        kw = dict(npicks=2, seeds=()) if entry == "maxmin" else dict(max_leaders=2, seeds=()) if entry == "leader" else \
            dict(rows=(1,)) if entry == "rowset_from_rows" else {}
        record("%s: 4128-bit rows" % entry, getattr(wide, entry)(**kw))
        record("%s: valid 4096-bit rows" % entry, getattr(widest, entry)(**kw))
        record("%s: valid empty table" % entry, getattr(empty, entry)(**EMPTY.get(entry, {})))
    record("bit_counts: valid empty table, a stale row set", empty.bit_counts(rs="stale"))
    for x in (wide, widest, empty):
        x.close()
    g = Graphs()
    for entry, cases in GRAPH_ENTRIES.items():
        for what, kw in cases.items():
            record("gsim_%s: %s" % (entry, what), getattr(g, entry)(**kw))
    return got
