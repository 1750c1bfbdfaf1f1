"""Popcount indexes on the GPU (gsim_popindex_*, gsim_db_search_bounded).  The index against the numpy rule (popindex_rule.py); every
result three ways -- gsim_db_search on the same handle byte for byte (hits, counts, approx), the oracle's scan of all rows, and the
index with and without the popcount-ordered copy of the rows against each other --; and the call's stats against the rule's
execution: the rows of every window, the number of stages, the route.  Everything is exact: no tolerances."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
import popindex_rule as R
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
NT = 16
KNOB = "GSIM_SUBSET_GATHER_MAX_PERMILLE"
TAN = dict()
TVS = [dict(metric=capi.METRIC_TVERSKY, alpha=a, beta=b) for a, b in ((1.0, 1.0), (1.0, 0.0), (0.5, 0.5), (0.3, 0.2), (2.0, 0.5))]
WIDTHS = [64, 128, 160, 896, 1024, 2048, 4096]
F32 = np.float32


@contextlib.contextmanager
def knob(value):
    """The gather knob is read once per handle, by gsim_db_create: set it around the creation of a table."""
    old = os.environ.get(KNOB)
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def table(db, base=0, permille=None):
    with knob(permille):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def pack(bits):
    """a 0/1 matrix (n, fp_bits) -> uint32 rows"""
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little").view(np.uint32).reshape(len(bits), bits.shape[1] // 32)


def uniform_rows(rng, n, W):
    """popcounts spread over [0, fp_bits]: every row has its own density; an all-zero and an all-one row at both ends and inside"""
    db = pack(rng.random((n, W * 32)) < rng.random(n)[:, None])
    db[[0, n // 3]] = 0
    db[[1, n - 1]] = 0xFFFFFFFF
    return db


def rows_of_popcount(rng, pops, W, inside=None, overlap=None):
    """one row per entry of pops with exactly that many bits; with `inside` (bit indices) and `overlap`, overlap[i] of row i's bits
    lie inside and the rest outside"""
    F = W * 32
    bits = np.zeros((len(pops), F), np.uint8)
    ins = np.zeros(F, bool)
    if inside is not None:
        ins[inside] = True
    for i, p in enumerate(pops):
        if inside is None:
            bits[i, rng.permutation(F)[:p]] = 1
        else:
            bits[i, rng.permutation(np.flatnonzero(ins))[:overlap[i]]] = 1
            bits[i, rng.permutation(np.flatnonzero(~ins))[:p - overlap[i]]] = 1
    return pack(bits)


def same_hits(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got["row"], want["row"]), what
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), what
    assert np.array_equal(got["common"], want["common"]) and np.array_equal(got["popc_db"], want["popc_db"]), what


class Case:
    """A table, its two indexes (without and with the copy of the rows) and the rule's view of it"""

    def __init__(self, db, base=0, permille=None, t=None, rule=None):
        self.db, self.base, self.permille = db, base, R.GATHER_PERMILLE if permille is None else permille
        self.t = t or table(db, base, permille)
        self.popc, self.order, self.first = rule or R.order_first(db, base)  # (rule: what an earlier case of the same table worked out)
        self.ix = {False: self.t.popindex(rows=False), True: self.t.popindex(rows=True)}

    def close(self):
        for ix in self.ix.values():
            ix.close()
        self.t.close()

    def check(self, queries, k, cutoff, kw, what, oracle=True, approx=True, want_stage=None):
        """One call per index against gsim_db_search (bytes), the oracle and the rule's stats; returns the rule's plans (copy index)."""
        queries = np.atleast_2d(queries)
        N = len(self.db)
        base_hits, base_approx = self.t.search(queries, k, cutoff, **kw)
        plans = None
        for copy, ix in self.ix.items():
            hits, ap, st = self.t.search_bounded(ix, queries, k, cutoff, approx=approx, stats=True, **kw)
            plans = [R.execute(q, self.db, self.popc, self.first, k, cutoff, kw, copy, approx, self.permille) for q in queries]
            want_st = R.expected_stats(plans)
            print(what, "copy" if copy else "no copy", "k", k, "cutoff", cutoff, {n: st[n] for n in want_st}, "rule", want_st,
                  [[(r, h) for r, h in p["scans"]] for p in plans])
            for i in range(len(queries)):
                assert hits[i].tobytes() == base_hits[i].tobytes(), (what, copy, i, "against gsim_db_search")
                if approx:
                    assert int(ap[i]) == int(base_approx[i]), (what, copy, i, int(ap[i]), int(base_approx[i]))
                    if cutoff <= 0:
                        assert int(ap[i]) == N
            assert {n: st[n] for n in want_st} == want_st, (what, copy)
            assert st["queries_one_stage"] + st["queries_two_stage"] + st["queries_plain"] == len(queries)
            assert st["launches"] >= 3 * sum(len(p["scans"]) for p in plans) and st["wall_ms"] > 0, (what, copy)
            if cutoff > 0 and st["queries_plain"] == 0 and all(p["rows_window"] < N for p in plans) and approx:
                assert st["rows_scanned"] == st["rows_window"] < N * len(queries), (what, copy)
            if want_stage is not None and want_stage.get(copy) is not None:
                assert [p["stage"] for p in plans] == [want_stage[copy]] * len(queries), (what, copy, [p["stage"] for p in plans])
        if oracle:
            for i, q in enumerate(queries):
                want, wap = O.search(q, self.db, k, cutoff, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0), self.base, NT)
                same_hits(base_hits[i], want[:k] if k else want[:0], (what, i, "oracle"))
                assert int(base_approx[i]) == wap, (what, i)
        return plans


# ---- the index ----

@pytest.mark.parametrize("bits", WIDTHS)
def test_order_and_first_equal_the_rule(bits):
    rng = np.random.default_rng(0x1D0 + bits)
    n, W = 3001, bits // 32
    db = uniform_rows(rng, n, W)
    popc, order, first = R.order_first(db)
    assert popc.min() == 0 and popc.max() == bits and first[-1] == n
    t = table(db)
    for rows in (False, True):
        with t.popindex(rows=rows) as ix:
            assert ix.order().tobytes() == order.tobytes(), (bits, rows)
            assert ix.first().tobytes() == first.tobytes() and ix.first().shape == (bits + 2,), (bits, rows)
    t.close()


def test_identical_rows_a_generated_table_a_row_base_and_an_attached_table():
    import torch
    W = 32
    same = np.tile(O.synth_rows(7, O.KIND_MORGAN, 0, 1, W), (4096, 1))
    t = table(same)
    with t.popindex() as ix:
        assert np.array_equal(ix.order(), np.arange(4096, dtype=np.uint32)), "equal popcounts: the rows in their own order"
        b = int(R.popcounts(same[:1])[0])
        first = ix.first()
        assert (first[:b + 1] == 0).all() and (first[b + 1:] == 4096).all()
    t.close()
    n, base = 5000, 1000000
    db = O.synth_rows(0x9E4, O.KIND_MORGAN, 0, n, W)
    g = capi.Table(W * 32).generate(0x9E4, capi.SYNTH_MORGAN, 0, n, 0)
    _, order, first = R.order_first(db)
    with g.popindex(rows=True) as ix:
        assert ix.order().tobytes() == order.tobytes() and ix.first().tobytes() == first.tobytes()
    g.set_row_base(base)
    with g.popindex() as ix:
        assert ix.order().tobytes() == (order + np.uint32(base)).tobytes() and ix.first().tobytes() == first.tobytes()
    g.close()
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), n, 0)
    c = Case(db, t=a)
    assert c.ix[True].order().tobytes() == order.tobytes() and c.ix[False].first().tobytes() == first.tobytes()
    c.check(db[[17, 4000]], 10, 0.0, TAN, "attached")
    c.check(db[[17, 4000]], 10, 0.6, TAN, "attached")
    c.close()
    del ten


# ---- the result rule ----

@pytest.mark.parametrize("shape", ["uniform", "morgan"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_the_result_is_gsim_db_searchs_byte_for_byte(bits, shape):
    rng = np.random.default_rng(0x2E5 + bits)
    n, W = 7003, bits // 32
    db = uniform_rows(rng, n, W) if shape == "uniform" else O.synth_rows(0xB17 + bits, O.KIND_MORGAN, 0, n, W)
    c = Case(db)
    # five queries, two of one popcount (a row and a shuffled copy of its bits would do; here: the same row twice), a zero query
    q = np.stack([db[11], db[n // 2], db[11], np.zeros(W, np.uint32), db[n - 2]])
    for k in (1, 64, 1000, n + 5):
        for cutoff in (0.0, 0.3, 0.7, 1.0):
            c.check(q, k, cutoff, TAN, (bits, shape))
    c.check(q[:2], 64, 0.3, TAN, (bits, shape, "no approx"), approx=False)
    c.check(q, 0, 0.3, TAN, (bits, shape, "k 0"))
    c.close()


@pytest.mark.parametrize("kw", TVS, ids=lambda kw: "%g-%g" % (kw["alpha"], kw["beta"]))
def test_tversky(kw):
    n, W = 7003, 32
    db = O.synth_rows(0x7E5, O.KIND_MORGAN, 0, n, W)
    c = Case(db)
    q = np.stack([db[5], db[n - 9], np.zeros(W, np.uint32)])
    for k, cutoff in ((10, 0.0), (10, 0.5), (2000, 0.5), (1, 1.0)):
        c.check(q, k, cutoff, kw, ("tversky", kw["alpha"], kw["beta"]))
    c.check(q, 10, 0.5, kw, ("tversky, no approx", kw["alpha"], kw["beta"]), approx=False)
    c.close()


# ---- windows and tables longer than the grids: every wave of the new kernels goes round its loop more than once ----
# (an MI355X has 256 compute units: the window scan runs 1024 waves, its lane kernel 2048, the popcount pass 4096)

def dense_rows(rng, n, W, lo=0.3, hi=0.8):
    """rows whose densities spread over [lo, hi], made in blocks"""
    out = np.empty((n, W), np.uint32)
    for r0 in range(0, n, 4096):
        m = min(4096, n - r0)
        d = (lo + (hi - lo) * rng.random(m, dtype=np.float32))[:, None]
        out[r0:r0 + m] = pack(rng.random((m, W * 32), dtype=np.float32) < d)
    return out


def query_and_planted(rng, db, a, nplant, max_cleared):
    """a query of exactly `a` bits; nplant rows of db, all over the table and in its last rows, become the query with a few bits cleared"""
    n, W = db.shape
    qbits = np.zeros(W * 32, np.uint8)
    qbits[rng.permutation(W * 32)[:a]] = 1
    where = np.unique(np.r_[rng.integers(0, n, nplant), n - 1, n - 2, 0])
    set_bits = np.flatnonzero(qbits)
    planted = np.tile(qbits, (len(where), 1))
    for i in range(len(where) - 1):  # (the table's last row stays the query itself: it is among the best hits whatever k)
        planted[i, rng.permutation(set_bits)[:int(rng.integers(0, max_cleared + 1))]] = 0
    db[where] = pack(planted)
    return pack(qbits[None, :])[0]


def long_window_case(db, q, cutoff, chunk_rows, waves, what):
    """The index against the rule, then the window of `cutoff` -- more than `waves` chunks of `chunk_rows` slots, and streamed -- and the
    narrowed and the unbounded query, with the copy, without it, and without it with the gather forced."""
    N, W = db.shape
    rule = None
    for permille in (None, 1000):
        c = Case(db, permille=permille, rule=rule)
        rule = c.popc, c.order, c.first
        if permille is None:
            assert c.ix[True].order().tobytes() == c.order.tobytes() and c.ix[False].order().tobytes() == c.order.tobytes(), what
            assert c.ix[True].first().tobytes() == c.first.tobytes(), what
        p = c.check(q, 100, cutoff, TAN, what)[0]
        assert p["scans"] == [("stream", p["window"])] and p["rows_scanned"] > waves * chunk_rows, (what, p["rows_scanned"], p["scans"])
        if permille == 1000:
            g = R.execute(q, db, c.popc, c.first, 100, cutoff, TAN, False, True, 1000)
            assert g["scans"] == [("gather", p["window"])], what
        hits, _ = c.t.search_bounded(c.ix[True], q, 100, cutoff)
        assert len(hits[0]) == 100 and hits[0]["row"].max() >= N - 2, "planted rows up to the table's last are among the hits"
        c.check(q, 100, cutoff, TAN, (what, "narrowed"), approx=False)
        c.check(np.stack([q, db[N // 2]]), 50, 0.0, TAN, (what, "no cutoff"))
        c.close()


def test_a_streamed_window_of_more_than_1024_chunks_at_4096_bits():
    """26 000 rows of 4096 bits (32 lanes a row: chunks of 16 slots); the window of cutoff 0.72 holds about 17 000"""
    rng = np.random.default_rng(0x10C4)
    db = dense_rows(rng, 26000, 128)
    q = query_and_planted(rng, db, 2048, 300, 500)
    long_window_case(db, q, 0.72, 16, 1024, "4096 bits")


def test_a_window_longer_than_the_lane_kernels_grid_at_160_bits():
    """300 000 rows of 160 bits (a slot per lane, 64 a chunk, 2048 waves; the popcount pass a row per lane, 4096 waves): the window of
    cutoff 0.72 holds about 200 000"""
    rng = np.random.default_rng(0x10C5)
    db = dense_rows(rng, 300000, 5)
    q = query_and_planted(rng, db, 80, 300, 20)
    long_window_case(db, q, 0.72, 64, 2048, "160 bits")


def test_a_table_longer_than_the_popcount_pass_and_its_window_at_128_bits():
    """2 200 000 rows of 128 bits (one lane a row: the popcount pass takes 512 rows a trip on 4096 waves, the window scan 512 slots a
    chunk on 1024): rows of about 16, 32, 64 and 96 bits, a query of 64, cutoff 0.6 -- the window holds about half the table"""
    rng = np.random.default_rng(0x10C6)
    n = 2200000
    r = rng.integers(0, 1 << 32, (3, n, 4), dtype=np.uint64).astype(np.uint32)
    kind = rng.integers(0, 4, n)[:, None]
    db = np.where(kind == 0, r[0], np.where(kind == 1, r[0] | r[1], np.where(kind == 2, r[0] & r[1], r[0] & r[1] & r[2])))
    del r
    q = query_and_planted(rng, db, 64, 300, 20)
    assert n > 4096 * 512, "the popcount pass goes round its loop"
    long_window_case(np.ascontiguousarray(db), q, 0.6, 512, 1024, "128 bits")


@pytest.mark.parametrize("bits", [256, 512, 1536, 8192])
def test_the_other_instantiations_and_the_wide_rows(bits):
    """two and four lanes a row; 1536 bits: no power-of-two lane count at 48 words (the popcount pass takes a row per wave, the scan a
    slot per lane); 8192 bits: 64 lanes a row and more popcounts than the LDS histogram has bins"""
    rng = np.random.default_rng(0x07E + bits)
    n, W = 5003, bits // 32
    db = uniform_rows(rng, n, W)
    c = Case(db)
    assert c.popc.min() == 0 and c.popc.max() == bits
    for copy in (False, True):
        assert c.ix[copy].order().tobytes() == c.order.tobytes() and c.ix[copy].first().tobytes() == c.first.tobytes(), (bits, copy)
    q = np.stack([db[11], db[n // 2], np.zeros(W, np.uint32)])
    for k, cutoff in ((64, 0.0), (64, 0.6), (1000, 0.9), (1, 1.0)):
        c.check(q, k, cutoff, TAN, (bits, "instantiations"))
    c.check(q[:2], 10, 0.6, TAN, (bits, "no approx"), approx=False)
    c.close()


# ---- boundaries of the bound ----

def test_a_bucket_exactly_at_the_cutoff_is_inside_and_one_ulp_above_it_is_outside():
    rng = np.random.default_rng(0xB0D)
    W = 2
    q = pack(np.r_[np.ones(10), np.zeros(54)][None, :])[0]
    inside = np.arange(10)
    # popcount 20 rows that hold the whole query (score 10 / 20 = 0.5 exactly), popcount 5 subsets (5 / 10), popcount 10 rows with 8
    # common bits (8 / 12), popcount 30 rows (at most 10 / 30) and the query itself
    pops = np.r_[np.full(40, 20), np.full(30, 5), np.full(50, 10), np.full(3000, 30), [10]]
    over = np.r_[np.full(40, 10), np.full(30, 5), np.full(50, 8), rng.integers(0, 11, 3000), [10]]
    db = rows_of_popcount(rng, pops, W, inside, over)
    db = db[rng.permutation(len(db))]
    c = Case(db)
    half, above = 0.5, float(np.nextafter(F32(0.5), F32(1)))
    ub = R.bounds(64, 10)
    assert ub[20] == F32(0.5) and ub[5] == F32(0.5) and ub[21] < F32(0.5) and ub[4] < F32(0.5)
    p = c.check(q, 200, half, TAN, "cutoff 0.5")[0]
    assert p["window"] == (5, 20) and p["rows_scanned"] == 40 + 30 + 50 + 1
    p = c.check(q, 200, above, TAN, "cutoff 0.5 + 1 ulp")[0]
    assert p["window"] == (6, 19) and p["rows_scanned"] == 50 + 1
    hits, approx = c.t.search(q, 200, half)
    assert int(approx[0]) == 121 and len(hits[0]) == 121
    hits, approx = c.t.search(q, 200, above)
    assert int(approx[0]) == 51
    c.close()


# ---- window geometry ----

@pytest.mark.parametrize("below", [700, 701])
def test_windows_of_every_length_around_a_chunk(below):
    """128-bit rows (one 16-byte lane a row: chunks of 512 slots), a query of 64 bits, cutoff 1.0: only the bucket of popcount 64
    passes.  `below` rows of a lower popcount put the window's first slot at either parity; the window ends at the order's last
    slot where no row has a higher popcount."""
    rng = np.random.default_rng(0x6E0 + below)
    W = 4
    qbits = np.zeros(128)
    qbits[rng.permutation(128)[:64]] = 1
    q = pack(qbits[None, :])[0]
    for m in (0, 1, 63, 64, 65, 511, 512, 513, 1025):
        for above in (0, 9000):
            pops = np.r_[rng.integers(0, 64, below), rng.integers(65, 129, above), rng.integers(0, 64, 9000 - above)]
            rest = rows_of_popcount(rng, pops, W)
            bucket = rows_of_popcount(rng, np.full(m, 64), W)
            bucket[::3] = q  # every third row of the bucket is the query itself
            db = np.concatenate([rest, bucket])
            db = db[rng.permutation(len(db))]
            c = Case(db)
            p = c.check(q, 1000, 1.0, TAN, ("geometry", below, m, above), want_stage={True: "one"})[0]
            assert p["rows_scanned"] == m and p["window"] == (64, 64)
            assert int(c.first[64]) == below + 9000 - above and (above > 0 or int(c.first[65]) == len(db))
            assert [r for r, _ in p["scans"]] == (["stream"] if m else [])
            hits, _ = c.t.search_bounded(c.ix[True], q, 1000, 1.0)
            assert len(hits[0]) == (m + 2) // 3
            c.close()


def test_windows_around_a_chunk_at_widths_that_take_other_loops():
    """the same at 1024 bits (eight lanes a row: chunks of 64 slots) and at 160 bits (one slot per lane)"""
    rng = np.random.default_rng(0x6E1)
    for bits, lengths in ((1024, (1, 63, 64, 65, 129)), (160, (1, 63, 64, 65, 200))):
        W = bits // 32
        a = bits // 2
        qbits = np.zeros(bits)
        qbits[rng.permutation(bits)[:a]] = 1
        q = pack(qbits[None, :])[0]
        for m in lengths:
            for below in (300, 301):
                pops = np.r_[rng.integers(0, a, below), rng.integers(a + 1, bits + 1, 3000)]
                bucket = rows_of_popcount(rng, np.full(m, a), W)
                bucket[::2] = q
                db = np.concatenate([rows_of_popcount(rng, pops, W), bucket])
                db = db[rng.permutation(len(db))]
                c = Case(db)
                p = c.check(q, 100, 1.0, TAN, ("geometry", bits, m, below))[0]
                assert p["rows_scanned"] == m and p["window"] == (a, a)
                c.close()


# ---- narrowing ----

def narrowing_table(rng):
    """128-bit rows, a query of bits 0 .. 29.  Bucket 30: the query itself (X, score 1), a row sharing 20 of its bits (Y, 20 / 40 = 0.5)
    and 4300 rows sharing at most 10 (at most 10 / 50); a subset of 15 of the query's bits (Z, 15 / 30 = 0.5, the same float) in a
    LOWER row than Y; 3000 rows of 76 .. 110 bits (bound below 0.4).  Stage 1's hull at k <= 1024 is bucket 30 alone."""
    W = 4
    q = pack(np.r_[np.ones(30), np.zeros(98)][None, :])[0]
    inside = np.arange(30)
    junk = rows_of_popcount(rng, np.full(4300, 30), W, inside, rng.integers(0, 11, 4300))
    far = rows_of_popcount(rng, rng.integers(76, 111, 3000), W)
    db = np.concatenate([junk, far])
    db = db[rng.permutation(len(db))]
    x, y, z = 100, 4000, 5
    db[x] = q
    db[y] = rows_of_popcount(rng, [30], W, inside, [20])[0]
    db[z] = rows_of_popcount(rng, [15], W, inside, [15])[0]
    return db, q, (x, y, z)


@pytest.mark.parametrize("permille", [None, 1000])
def test_one_stage_two_stages_the_tie_outside_the_hull_and_too_few_hits(permille):
    """permille 1000: the index without the copy gathers every window (under the default it hands windows of this size to the plain scan)"""
    rng = np.random.default_rng(0x57A)
    db, q, (x, y, z) = narrowing_table(rng)
    c = Case(db, permille=permille)
    nocopy = "plain" if permille is None else None
    # k = 1: the query's own row, every other bucket's bound is below 1: final after stage 1
    p = c.check(q, 1, 0.0, TAN, "one stage", want_stage={False: nocopy or "one", True: "one"})[0]
    assert p["scans"] == [("stream", (30, 30))]
    # k = 2: stage 1 returns X and Y; Z, outside the hull, ties Y's 0.5 in a lower row: bucket 15's bound is not BELOW s_k, stage 2 runs
    p = c.check(q, 2, 0.0, TAN, "the tie", want_stage={False: nocopy or "two", True: "two"})[0]
    assert [h for _, h in p["scans"]] == [(30, 30), (15, 60)]
    hits, _ = c.t.search_bounded(c.ix[True], q, 2, 0.0)
    assert hits[0]["row"].tolist() == [x, z] and hits[0]["score"].tolist() == [1.0, 0.5], "the lower row of the tie displaces Y"
    # k = 20: the 20th best of bucket 30 scores at most 0.2, a score every bucket's bound reaches: stage 2 wants (nearly) the whole
    # order, which is past the streaming limit -- the plain scan answers
    c.check(q, 20, 0.0, TAN, "stage 2 past the route limit", want_stage={False: nocopy, True: "plain"})
    # cutoff 0.4 without approx, k = 3: stage 1 finds X and Y only -- fewer than k -- and stage 2 rescans the whole cutoff window
    p = c.check(q, 3, 0.4, TAN, "too few hits", approx=False, want_stage={False: nocopy or "two", True: "two"})[0]
    assert [h for _, h in p["scans"]] == [(30, 30), p["window"]] and p["window"] == (12, 75)
    hits, ap = c.t.search_bounded(c.ix[True], q, 3, 0.4, approx=False)
    assert ap is None and hits[0]["row"].tolist() == [x, z, y]
    # ... with approx the cutoff window is scanned once, whole
    c.check(q, 3, 0.4, TAN, "approx wanted", want_stage={False: nocopy or "one", True: "one"})
    c.close()


def test_narrowing_on_a_morgan_table():
    n, W = 20000, 32
    db = O.synth_rows(0x4A2, O.KIND_MORGAN, 0, n, W)
    rng = np.random.default_rng(0x4A2)
    c = Case(db)
    q = np.stack([db[77], db[19999], pack(rng.random((1, 1024)) < 0.05)[0], pack(rng.random((1, 1024)) < 0.5)[0]])
    plans = c.check(q[:2], 1, 0.0, TAN, "morgan k 1", want_stage={True: "one"})
    assert all(p["rows_scanned"] < n // 2 for p in plans), "a row of the table as the query: one stage over a few buckets"
    c.check(q, 10, 0.0, TAN, "morgan")
    c.check(q, 1000, 0.0, TAN, "morgan k 1000")
    c.check(q, 64, 0.5, TAN, "morgan cutoff", approx=False)
    c.close()


# ---- state and lifetime ----

def test_the_search_state_is_left_as_it_was_found_and_the_destroy_order():
    n, W = 7003, 32
    db = O.synth_rows(0x57E, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    q = db[[3, 500, 6000]]
    before = [t.search(q[i], k, cut) for i in range(3) for k, cut in ((10, 0.0), (9000, 0.0), (100, 0.4))]
    ix = t.popindex(rows=True)
    ix2 = t.popindex()
    for k, cut in ((10, 0.0), (9000, 0.3), (100, 0.6), (0, 0.0)):
        first = [t.search_bounded(i, q, k, cut) for i in (ix, ix2)]
        again = [t.search_bounded(i, q, k, cut) for i in (ix, ix2)]
        for (h1, a1), (h2, a2) in zip(first, again):
            assert b"".join(h.tobytes() for h in h1) == b"".join(h.tobytes() for h in h2) and a1.tobytes() == a2.tobytes(), "from run to run"
    after = [t.search(q[i], k, cut) for i in range(3) for k, cut in ((10, 0.0), (9000, 0.0), (100, 0.4))]
    for (h1, a1), (h2, a2) in zip(before, after):
        assert h1[0].tobytes() == h2[0].tobytes() and a1.tobytes() == a2.tobytes()
    other = table(db[:100])
    with pytest.raises(capi.GsimError) as e:
        other.search_bounded(ix, q, 5)
    assert e.value.code == -1 and "another handle" in str(e.value)
    other.close()
    ix.close()
    hits, _ = t.search_bounded(ix2, q, 5)  # one index goes, the other still serves
    assert hits[0]["row"][0] == 3
    ix2.close()
    ix2.close()  # (closing twice is harmless)
    t.close()
    # an empty table has an index too
    e = capi.Table(64).add_rows(np.zeros((0, 2), np.uint32)).finalize(0, 1)
    with e.popindex(rows=True) as eix:
        assert len(eix.order()) == 0 and not eix.first().any()
        hits, ap, st = e.search_bounded(eix, np.ones((2, 2), np.uint32), 5, stats=True)
        assert [len(h) for h in hits] == [0, 0] and ap.tolist() == [0, 0] and st["rows_scanned"] == 0
    e.close()
