"""The case list of the row-hash calls (gsim_rowhash_*, gsim_row_hash, gsim_duplicates), recorded by
scripts/make_front_errors_golden.py (list "rowhash") into tests/golden/rowhash_front_errors.json and replayed by
tests/test_rowhash_host.py: on tables that are not on a GPU, one argument changed at a time from a valid call, and a handful of
valid calls (a state error: the tables have no rows on a GPU; GSIM_OK for the host functions and for the calls that read the index
alone).  `run_all()` returns {case id: {code, message, out}} as single_front_errors_cases.py does.

An index cannot be made without a GPU.  Where a front reads one before any device state, the cases pass a stand-in: zeroed memory
that begins as gsim_rowhash does (capi_internal.h), with the owner and the row count the case asks for."""
import ctypes as C

from front_errors_cases import host_table, merged
from gpusimilarity_amd import capi
from single_front_errors_cases import ROWS, U32P, U64P, Calls


class FakeRowhash(C.Structure):
    _fields_ = [("owner", C.c_void_p), ("device", C.c_int), ("nrows", C.c_uint64), ("fp_bits", C.c_uint32), ("row_base", C.c_uint32),
                ("flags", C.c_uint32), ("rest", C.c_uint8 * 512)]


class HashCalls(Calls):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.narrow = host_table(self.bits // 2, 3)

    def close(self):
        super().close()
        self.narrow.close()

    def index(self, ix):
        """None, or a stand-in index: "mine" (owner: the table), "stale" (the table, another row count), "empty" (no rows)"""
        if ix is None:
            return None
        f = FakeRowhash()
        f.owner = self.t._h.value
        f.nrows = 0 if ix == "empty" else self.rows + (5 if ix == "stale" else 0)
        f.fp_bits = self.bits
        self.keep.append(f)
        return C.cast(C.byref(f), C.c_void_p)

    def rowhash_create(self, db=True, flags=0, out=True, base=0):
        L = capi.load()
        L.gsim_db_set_row_base(self.t._h, base)
        r = self.graph(lambda o: L.gsim_rowhash_create(self.db(db), flags, o), out)
        L.gsim_db_set_row_base(self.t._h, 0)
        return r

    def rowhash_get_stats(self, ix="mine", stats=True):
        return self.seen(capi.load().gsim_rowhash_get_stats(self.index(ix), self.stats(capi.GsimRowhashStats, stats)))

    def rowhash_groups(self, ix="empty", first=True, size=True):
        return self.seen(capi.load().gsim_rowhash_groups(self.index(ix), self.out("first", first, 4 * self.rows), self.out("size", size, 4 * self.rows)))

    def rowhash_rowset(self, ix="mine", flags=0, out=True):
        return self.graph(lambda o: capi.load().gsim_rowhash_rowset(self.index(ix), flags, o), out)

    def rowhash_find(self, ix="mine", queries=True, nq=2, row=True, size=True):
        q = self.inp([[1] * self.W] * max(nq, 1), "uint32", U32P) if queries else None
        return self.seen(capi.load().gsim_rowhash_find(self.index(ix), q, nq, self.out("row", row, 4 * max(nq, 1)), self.out("size", size, 4 * max(nq, 1))))

    def rowhash_find_db(self, ix="mine", left="other", begin=0, end=3, row=True, size=True):
        h = {None: None, "other": self.other._h, "own": self.t._h, "narrow": self.narrow._h}[left]
        return self.seen(capi.load().gsim_rowhash_find_db(self.index(ix), h, begin, end, self.out("row", row, 4 * ROWS), self.out("size", size, 4 * ROWS)))

    def rowhash_destroy(self):
        return self.seen(capi.load().gsim_rowhash_destroy(None))

    def row_hash(self, rows=True, nrows=2, fp_bits=64, hash=True):
        r = self.inp([[1, 2], [2, 1]], "uint32", U32P) if rows else None
        return self.seen(capi.load().gsim_row_hash(r, nrows, fp_bits, self.out("hash", hash, 16, U64P)))

    def duplicates(self, rows=True, nrows=3, fp_bits=64, first=True, size=True, ngroups=True):
        r = self.inp([[1, 2], [2, 1], [1, 2]], "uint32", U32P) if rows else None
        return self.seen(capi.load().gsim_duplicates(r, nrows, fp_bits, self.out("first", first, 12), self.out("size", size, 12),
                                                     self.out("ngroups", ngroups, 8, U64P)))


def nulls(*names):
    return {"NULL " + n: {n: False if n not in ("ix", "left") else None} for n in names}


WIDTHS = {"fp_bits 0": dict(fp_bits=0), "fp_bits 33": dict(fp_bits=33), "fp_bits 32800": dict(fp_bits=32800)}
ENTRIES = {
    "rowhash_create": {"NULL db": dict(db=False), "NULL out": dict(out=False), "unknown flags": dict(flags=1), "the top flag bit": dict(flags=0x80000000),
                       "a row base that takes the last row to GSIM_ROW_NONE": dict(base=0xFFFFFFFF - ROWS + 1),
                       "valid": dict(), "valid the largest row base": dict(base=0xFFFFFFFF - ROWS)},
    "rowhash_get_stats": merged(nulls("ix", "stats"), {"valid": dict()}),
    "rowhash_groups": merged(nulls("ix"), {"both first and size NULL": dict(first=False, size=False), "valid": dict(),
                                           "valid first alone": dict(size=False), "valid size alone": dict(first=False)}),
    "rowhash_rowset": merged(nulls("ix", "out"), {"unknown flags": dict(flags=2), "all flags": dict(flags=0xFFFFFFFF), "valid": dict(),
                                                  "valid the repeats": dict(flags=1), "valid index of another row count": dict(ix="stale")}),
    "rowhash_find": merged(nulls("ix", "queries", "row"), {"valid": dict(), "valid NULL size": dict(size=False), "valid nq 0": dict(nq=0),
                                                           "valid NULL queries and row with nq 0": dict(nq=0, queries=False, row=False),
                                                           "valid index of another row count": dict(ix="stale")}),
    "rowhash_find_db": merged(nulls("ix", "left", "row"), {
        "a range past the left rows": dict(end=4), "begin past end": dict(begin=2, end=1), "a left table of other fp_bits": dict(left="narrow"),
        "valid": dict(), "valid NULL size": dict(size=False), "valid the table itself": dict(left="own", end=ROWS),
        "valid an empty range with NULL row": dict(begin=2, end=2, row=False), "valid index of another row count": dict(ix="stale")}),
    "rowhash_destroy": {"valid NULL": dict()},
    "row_hash": merged(nulls("rows", "hash"), WIDTHS, {"2^32 - 1 rows": dict(nrows=0xFFFFFFFF), "valid": dict(),
                                                      "valid no rows": dict(nrows=0, rows=False, hash=False)}),
    "duplicates": merged(nulls("rows"), WIDTHS, {"2^32 - 1 rows": dict(nrows=0xFFFFFFFF), "valid": dict(), "valid first alone": dict(size=False, ngroups=False),
                                                 "valid the count alone": dict(first=False, size=False), "valid no rows": dict(nrows=0, rows=False)}),
}
# the calls that answer without a device: the host functions, and those that read nothing but the index
ANSWERED = ("rowhash_get_stats", "rowhash_groups", "rowhash_destroy", "row_hash", "duplicates")


def run_all():
    L = capi.load()
    got = {}
    c = HashCalls(bits=1024, rows=ROWS)
    for entry, cases in ENTRIES.items():
        for what, kw in cases.items():
            code, out = getattr(c, entry)(**kw)
            got["%s: %s" % (entry, what)] = {"code": int(code), "message": L.gsim_last_error().decode() if code != 0 else "", "out": out}
    c.close()
    return got
