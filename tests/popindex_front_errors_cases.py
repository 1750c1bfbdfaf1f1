"""The case list of the popcount-index calls (gsim_popindex_*, gsim_popcount_bounds, gsim_db_search_bounded), recorded by
scripts/make_front_errors_golden.py (list "popindex") into tests/golden/popindex_front_errors.json and replayed by
tests/test_popindex_host.py: on tables that are not on a GPU, one argument changed at a time from a valid call, and a handful of
valid calls (a state error: the tables have no rows on a GPU; GSIM_OK for the host function).  `run_all()` returns
{case id: {code, message, out}} as single_front_errors_cases.py does.

An index cannot be made without a GPU.  Where a front reads one before any device state, the cases pass a stand-in: zeroed memory
that begins as gsim_popindex does (capi_internal.h), with the owner and the row count the case asks for."""
import ctypes as C

from front_errors_cases import merged
from gpusimilarity_amd import capi
from single_front_errors_cases import FP, ROWS, TAN, TV, U32P, U64P, Calls

nan = float("nan")


class FakePopindex(C.Structure):
    _fields_ = [("owner", C.c_void_p), ("device", C.c_int), ("nrows", C.c_uint64), ("fp_bits", C.c_uint32), ("row_base", C.c_uint32),
                ("flags", C.c_uint32), ("rest", C.c_uint8 * 256)]


class PopCalls(Calls):
    def index(self, ix):
        """None, or a stand-in index: "mine" (owner: the table), "other" (another handle), "stale" (the table, another row count)"""
        if ix is None:
            return None
        f = FakePopindex()
        f.owner = (self.other if ix == "other" else self.t)._h.value
        f.nrows = self.rows + (5 if ix == "stale" else 0)
        f.fp_bits = self.bits
        self.keep.append(f)
        return C.cast(C.byref(f), C.c_void_p)

    def popindex_create(self, db=True, flags=0, out=True):
        return self.graph(lambda o: capi.load().gsim_popindex_create(self.db(db), flags, o), out)

    def popindex_first(self, ix="mine", first=True):
        return self.seen(capi.load().gsim_popindex_first(self.index(ix), self.out("first", first, 8 * (self.bits + 2), U64P)))

    def popindex_order(self, ix="mine", order=True):
        return self.seen(capi.load().gsim_popindex_order(self.index(ix), self.out("order", order, 4 * self.rows)))

    def popindex_destroy(self):
        return self.seen(capi.load().gsim_popindex_destroy(None))

    def popcount_bounds(self, fp_bits=32, popc=3, metric=TAN, alpha=1.0, beta=1.0, ub=True):
        return self.seen(capi.load().gsim_popcount_bounds(fp_bits, popc, metric, alpha, beta, self.out("ub", ub, 4 * 33, FP)))

    def search_bounded(self, db=True, ix="mine", queries=True, nq=2, k=5, cutoff=0.0, metric=TAN, alpha=1.0, beta=1.0, hits=True, counts=True,
                       approx=True, stats=True):
        q = self.inp([[1] * self.W] * max(nq, 1), "uint32", U32P) if queries else None
        return self.seen(capi.load().gsim_db_search_bounded(self.db(db), self.index(ix), q, nq, k, cutoff, metric, alpha, beta,
                                                            self.out("hits", hits, 12 * max(k, 1) * max(nq, 1), None),
                                                            self.out("counts", counts, 4 * max(nq, 1)),
                                                            self.out("approx", approx, 8 * max(nq, 1), U64P),
                                                            self.stats(capi.GsimPopindexStats, stats)))


def nulls(*names):
    return {"NULL " + n: {n: False if n != "ix" else None} for n in names}


ENTRIES = {
    "popindex_create": {"NULL db": dict(db=False), "NULL out": dict(out=False), "unknown flags": dict(flags=2),
                        "unknown flag bits beside the known one": dict(flags=3), "the top flag bit": dict(flags=0x80000000),
                        "valid": dict(), "valid with the copy of the rows": dict(flags=1)},
    "popindex_first": {"NULL ix": dict(ix=None), "NULL first": dict(first=False)},
    "popindex_order": {"NULL ix": dict(ix=None), "NULL order": dict(order=False)},
    "popindex_destroy": {"valid NULL": dict()},
    "popcount_bounds": {"NULL ub": dict(ub=False), "fp_bits 0": dict(fp_bits=0), "fp_bits 33": dict(fp_bits=33), "fp_bits 32800": dict(fp_bits=32800),
                        "popcount above fp_bits": dict(popc=33), "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
                        "valid": dict(), "valid popcount 0": dict(popc=0), "valid popcount fp_bits": dict(popc=32),
                        "valid Tversky 1 0": dict(metric=TV, alpha=1.0, beta=0.0), "valid Tversky NaN alpha": dict(metric=TV, alpha=nan, beta=0.5)},
    "search_bounded": merged(nulls("db", "ix", "queries", "hits", "counts"), {
        "unknown metric": dict(metric=7), "negative metric": dict(metric=-1), "an index made for another handle": dict(ix="other"),
        "valid": dict(), "valid NULL approx": dict(approx=False), "valid NULL stats": dict(stats=False), "valid k 0": dict(k=0),
        "valid nq 0": dict(nq=0), "valid cutoff": dict(cutoff=0.7), "valid Tversky .3 .2": dict(metric=TV, alpha=0.3, beta=0.2),
        "valid Tversky NaN alpha": dict(metric=TV, alpha=nan, beta=0.5), "valid index of another row count": dict(ix="stale")}),
}


def run_all():
    L = capi.load()
    got = {}
    c = PopCalls(bits=1024, rows=ROWS)
    for entry, cases in ENTRIES.items():
        for what, kw in cases.items():
            code, out = getattr(c, entry)(**kw)
            got["%s: %s" % (entry, what)] = {"code": int(code), "message": L.gsim_last_error().decode() if code != 0 else "", "out": out}
    c.close()
    return got
