"""Exact k-nearest-neighbour lists on the GPU (gsim_db_knn).

Expected values: list i = oracle_lib.search(row i, table, k + 1, cutoff, ...) minus row i, cut to k -- the rule's first sentence
(include/gpusim_hip.h), test_gpu_neighbors.py's oracle_lists with k + 1.  Indices are compared exactly and scores by their bits:
no tolerances anywhere.

Non-vacuity, asserted on the EXPECTED result: a compared case at the smallest cutoff has at least 5 full lists whose boundary tie
group is cut (the candidate after the k-th scores the same as the k-th: found with a k + 2 search) and exactly the planted all-zero
row's list empty; a compared case with a biting cutoff has at least 5 non-empty lists shorter than k.  Sparse rows wider than 128
bits have no pair above 0.15, so a biting cutoff is only used on the sparse 128-bit table and on Morgan tables.

The parity tables are test_gpu_neighbors.py's (same seeds, the same duplicate of row 5 and all-zero row) with five more copies of
row 5 behind the first: without them the dense tables have too few cut ties at k = 1 (2 at 1024 bits, 4 at 896; 9 at 2048 bits with
k = 5) for the condition above, with them every case has the seven lists of the copies at least.  Fewest cut ties, measured on the
CPU with the oracle: 9, dense 1024-bit rows at k = 1.  At cutoff 0.3 and k = 5: sparse 128-bit 460 short lists and 732 empty,
Morgan 1024-bit 37 short, Morgan 4096-bit 6 short; Morgan 128-bit rows have no short list at 0.3, so that table is cut at 0.5
(222 short)."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from gpusimilarity_amd.fingerprintdb import FingerprintDB

pytestmark = pytest.mark.gpu
NT = 16
PAIRS = "GSIM_KNN_LAUNCH_PAIRS"
TINY = float(np.nextafter(np.float32(0), np.float32(1)))  # the smallest positive float: "every row with a non-zero score"
TAN = dict()
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
COL_TILE = 256


@contextlib.contextmanager
def knobs(**values):
    """The knobs are read once per handle, by gsim_db_create: set them around the creation of a table."""
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def table(db, pairs=None, base=0):
    with knobs(**{PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def oracle_hits(db, k, cutoff, kw=TAN, rows=None):
    """row i -> the hits of oracle_lib.search(row i, table, k, cutoff, ...) with row i's own hit removed"""
    def one(i):
        hits, _ = O.search(db[i], db, k, cutoff, kw.get("metric", O.METRIC_TANIMOTO), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        return hits[hits["row"] != i]
    with ThreadPoolExecutor(NT) as pool:
        return list(pool.map(one, range(len(db)) if rows is None else rows))


def expected(db, k, cutoff, kw=TAN, rows=None, base=0):
    """-> CSR of the rule: search(k + 1) minus the row, cut to k"""
    lists = [h[:k] for h in oracle_hits(db, k + 1, cutoff, kw, rows)]
    indptr = np.zeros(len(lists) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(h) for h in lists])
    cat = np.concatenate(lists) if lists else np.zeros(0, O.HIT_DTYPE)
    return indptr, cat["row"].astype(np.uint32) + np.uint32(base), cat["score"].astype(np.float32)


def counts(csr):
    return np.diff(csr[0].astype(np.int64))


def tie_cuts(db, k, cutoff, kw=TAN):
    """full lists whose boundary tie group is cut: among search(k + 2) minus the row, entry k scores the same as entry k - 1"""
    return sum(1 for h in oracle_hits(db, k + 2, cutoff, kw) if len(h) > k and h["score"][k] == h["score"][k - 1])


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indptr")
    assert np.array_equal(got[1], want[1]), (what, "indices")
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (what, "scores")


def as_bytes(csr):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in csr)


def planted(seed, kind, n, W):
    db = O.synth_rows(seed, kind, 0, n, W)
    db[n // 3:n // 3 + 6] = db[5]  # duplicates: score 1.0; seven identical rows, so their lists are cut inside a tie at k = 1 and k = 5
    db[n // 2] = 0                 # an all-zero row: an empty list, and in nobody's list
    return db


WIDTHS = [128, 160, 256, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    """n = 1200 (700 dense): four full owner tiles and one of 176 rows, whose last wave has 48."""
    W = bits // 32
    n = 1200 if kind != O.KIND_DENSE else 700
    db = planted(0xBE11 + bits + 7 * kind, kind, n, W)
    t = table(db)
    for kw in (TAN, TV):
        for k in (1, 5, 128):
            what = (bits, kind, kw, k)
            want = expected(db, k, TINY, kw)
            cuts = tie_cuts(db, k, TINY, kw)
            empty = np.flatnonzero(counts(want) == 0)
            print(what, "full", int((counts(want) == k).sum()), "tie cuts", cuts, "empty", empty.tolist())
            assert cuts >= 5 and empty.tolist() == [n // 2], what
            st = {}
            got = t.knn(k, TINY, stats=st, **kw)
            same(got, want, what)
            assert st["rows"] == n and st["pairs"] == n * n and st["entries"] == len(got[1]) and st["launches"] >= 1, st
            assert st["inserts"] >= st["entries"], st
    t.close()


BITING = [(128, O.KIND_SPARSE, TAN, 0.3), (128, O.KIND_SPARSE, TV, 0.5), (128, O.KIND_MORGAN, TAN, 0.5), (1024, O.KIND_MORGAN, TAN, 0.3),
          (4096, O.KIND_MORGAN, TAN, 0.3), (4096, O.KIND_MORGAN, TV, 0.3)]


@pytest.mark.parametrize("bits,kind,kw,cutoff", BITING)
def test_parity_with_a_biting_cutoff(bits, kind, kw, cutoff):
    n, k = 1200, 5
    db = planted(0xBE11 + bits + 7 * kind, kind, n, bits // 32)
    want = expected(db, k, cutoff, kw)
    c = counts(want)
    print(bits, kind, kw, cutoff, "full", int((c == k).sum()), "short", int(((c > 0) & (c < k)).sum()), "empty", int((c == 0).sum()))
    assert int(((c > 0) & (c < k)).sum()) >= 5, (bits, kind, kw)
    t = table(db)
    same(t.knn(k, cutoff, **kw), want, (bits, kind, kw, cutoff))
    t.close()


@pytest.mark.parametrize("bits", [1024, 256])
def test_asymmetric_tversky(bits):
    """The owner row is the query: a = popc(row i) takes alpha, b = popc(row j) takes beta."""
    n, k = 1200, 5
    db = planted(0xA5E + bits, O.KIND_MORGAN, n, bits // 32)
    t = table(db)
    for alpha, beta in ((0.3, 0.7), (1.0, 0.0)):
        kw = dict(metric=capi.METRIC_TVERSKY, alpha=alpha, beta=beta)
        want = expected(db, k, TINY, kw)
        flipped = expected(db, k, TINY, dict(kw, alpha=beta, beta=alpha))
        assert tie_cuts(db, k, TINY, kw) >= 5 and np.flatnonzero(counts(want) == 0).tolist() == [n // 2]
        assert not np.array_equal(want[1], flipped[1]), "the weights' roles matter on this table"
        same(t.knn(k, TINY, **kw), want, (bits, alpha, beta))
    t.close()


def test_fewer_rows_than_k():
    W = 32
    db = O.synth_rows(0xFE3, O.KIND_MORGAN, 0, 40, W)
    db[20] = 0
    want = expected(db, 128, TINY)
    assert counts(want).max() <= 39 and int((counts(want) > 0).sum()) == 39
    t = table(db)
    got = t.knn(128, TINY)
    same(got, want, "n = 40, k = 128")
    t.close()
    for n in (1, 2, 65, 257):
        db = O.synth_rows(0xFE3 + n, O.KIND_MORGAN, 0, n, W)
        t = table(db)
        got = t.knn(5, TINY)
        same(got, expected(db, 5, TINY), n)
        assert len(got[0]) == n + 1
        if n == 1:
            assert got[0].tolist() == [0, 0] and len(got[1]) == 0
        t.close()


@pytest.mark.parametrize("k", [1, 7, 128])
def test_ties_and_self_exclusion(k):
    """600 rows that are copies of 3 distinct fingerprints, interleaved: 270 copies each of two of them, 60 of the third.  Row i's
    list is the k lowest-numbered other copies of its fingerprint at 1.0 -- never row i -- then, for the rare fingerprint at
    k = 128, the next score group's lowest rows."""
    n, W = 600, 32
    fps = O.synth_rows(0x71E5, O.KIND_MORGAN, 0, 3, W)
    which = np.array([2 if r % 10 == 9 else (r - r // 10) % 2 for r in range(n)])
    assert np.bincount(which).tolist() == [270, 270, 60]
    db = fps[which]
    want = expected(db, k, TINY)
    indptr, indices, scores = want
    for i in range(n):
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        copies = [j for j in np.flatnonzero(which == which[i]).tolist() if j != i]
        m = min(k, len(copies))
        assert indices[lo:lo + m].tolist() == copies[:m] and (scores[lo:lo + m] == 1.0).all() and i not in indices[lo:hi]
        assert hi - lo == k and (scores[lo + m:hi] < 1.0).all()
        if m < k:  # the next score group: one other fingerprint, its lowest rows
            nxt = which[indices[lo + m]]
            assert indices[lo + m:hi].tolist() == np.flatnonzero(which == nxt)[:k - m].tolist()
    assert (k > 59) == bool((scores < 1.0).any())
    t = table(db)
    same(t.knn(k, TINY), want, k)
    t.close()


def test_cutoff_equal_to_scores_that_occur():
    """cutoff 0.5 with c / (a + b - c) = 1/2 pairs present: they are listed (>=); RN(1/3) pairs at cutoff RN(1/3)."""
    n, W, k = 900, 32, 5
    db = O.synth_rows(0x7133, O.KIND_SPARSE, 0, n, W)

    def bits(*ranges):
        x = np.zeros(W * 32, np.uint8)
        for lo, hi in ranges:
            x[lo:hi] = 1
        return np.packbits(x, bitorder="little").view(np.uint32)

    db[10] = bits((0, 40))             # 40 bits
    db[11] = bits((0, 20))             # vs 10: c = 20, a + b - c = 40: exactly 1/2
    db[12] = bits((0, 10), (40, 50))   # vs 11: c = 10, a + b - c = 30: RN(1/3)
    t = table(db)
    for cutoff in (np.float32(0.5), np.float32(1.0) / np.float32(3.0)):
        want = expected(db, k, float(cutoff))
        assert (want[2] == cutoff).any() and len(want[1]) >= 2, cutoff
        same(t.knn(k, float(cutoff)), want, cutoff)
        above = float(np.nextafter(cutoff, np.float32(2)))
        fewer = expected(db, k, above)
        assert len(fewer[1]) < len(want[1])
        same(t.knn(k, above), fewer, above)
    t.close()


def test_the_result_does_not_depend_on_the_launch_cut():
    n, W, k = 1200, 32, 5
    db = planted(0xC07, O.KIND_MORGAN, n, W)
    want = expected(db, k, TINY)
    whole = table(db)
    st0 = {}
    a = whole.knn(k, TINY, stats=st0)
    same(a, want, "default plan")
    whole.close()
    ntiles = -(-n // COL_TILE)
    for pairs, launches in ((1, ntiles), (n * 2 * COL_TILE, -(-ntiles // 2))):
        cut = table(db, pairs=pairs)  # (a launch never covers less than one column tile)
        st = {}
        b = cut.knn(k, TINY, stats=st)
        assert st["launches"] == launches > st0["launches"], (st, st0)
        assert as_bytes(b) == as_bytes(a), pairs
        assert st["inserts"] == st0["inserts"] and st["pairs"] == st0["pairs"] == n * n
        big = cut.knn(128, TINY, **TV)
        cut.close()
        ref = table(db)
        assert as_bytes(big) == as_bytes(ref.knn(128, TINY, **TV)), pairs
        ref.close()


def test_ranges_and_the_row_base():
    n, W, k, base = 1200, 32, 5, 1000
    db = planted(0xC08, O.KIND_MORGAN, n, W)
    t = table(db)
    full = t.knn(k, TINY)
    same(full, expected(db, k, TINY), "full")
    ind, sc, cnt = [], [], []
    for lo, hi in ((0, 300), (300, 301), (301, n)):
        st = {}
        p_indptr, p_ind, p_sc = t.knn(k, TINY, row_begin=lo, row_end=hi, stats=st)
        assert len(p_indptr) == hi - lo + 1 and st["rows"] == hi - lo and st["pairs"] == (hi - lo) * n
        assert np.array_equal(p_indptr.astype(np.int64), full[0][lo:hi + 1].astype(np.int64) - int(full[0][lo]))
        ind.append(p_ind)
        sc.append(p_sc)
    assert np.array_equal(np.concatenate(ind), full[1])
    assert np.array_equal(np.concatenate(sc).view(np.uint32), full[2].view(np.uint32))
    empty = t.knn(k, TINY, row_begin=17, row_end=17)
    assert empty[0].tolist() == [0] and len(empty[1]) == 0 and len(empty[2]) == 0
    t.set_row_base(base)
    based = t.knn(k, TINY)
    assert np.array_equal(based[0], full[0]) and np.array_equal(based[1], full[1] + np.uint32(base))
    assert np.array_equal(based[2].view(np.uint32), full[2].view(np.uint32))
    part = t.knn(k, TINY, row_begin=999, row_end=1100)
    assert np.array_equal(part[1], full[1][int(full[0][999]):int(full[0][1100])] + np.uint32(base))
    t.close()


@pytest.mark.parametrize("k", [5, 128])
def test_against_the_neighbour_lists(k):
    """Every kNN list = the first k entries of that row's gsim_db_neighbors list re-sorted by (score descending, column)."""
    n, W, cutoff = 1200, 32, 0.5
    db = planted(0xC09, O.KIND_MORGAN, n, W)
    t = table(db)
    indptr, indices, scores = t.neighbors(cutoff)
    got = t.knn(k, cutoff)
    t.close()
    nonempty = 0
    for i in range(n):
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        cols, sc = indices[lo:hi], scores[lo:hi]
        o = np.lexsort((cols, -sc.astype(np.float64)))[:k]
        a, b = int(got[0][i]), int(got[0][i + 1])
        assert np.array_equal(got[1][a:b], cols[o]), i
        assert np.array_equal(got[2][a:b].view(np.uint32), sc[o].view(np.uint32)), i
        nonempty += b > a
    assert nonempty >= 100


def test_the_graph_object_and_the_wrapper():
    """The result is a gsim_graph of its own kind: the join accessor refuses it, the totals are in gsim_graph_get_stats."""
    import ctypes as C
    n, W, k = 300, 32, 5
    db = planted(0xC0A, O.KIND_MORGAN, n, W)
    t = table(db)
    L = capi.load()
    g = C.c_void_p()
    assert L.gsim_db_knn(t._h, k, TINY, 0, 1.0, 1.0, 0, n, C.byref(g)) == 0 and g.value
    js, gs, ks = capi.GsimJoinStats(), capi.GsimGraphStats(), capi.GsimKnnStats()
    assert L.gsim_graph_get_join_stats(g, C.byref(js)) == -1
    assert L.gsim_graph_get_stats(g, C.byref(gs)) == 0 and L.gsim_graph_get_knn_stats(g, C.byref(ks)) == 0
    rows, nnz = C.c_uint64(0), C.c_uint64(0)
    assert L.gsim_graph_shape(g, C.byref(rows), C.byref(nnz)) == 0 and rows.value == n
    assert gs.launches == ks.launches >= 1 and gs.pairs == ks.entries == nnz.value and ks.rows == n and ks.pairs == n * n
    assert ks.kernel_ms > 0 and ks.wall_ms > 0 and ks.clock_mhz > 100
    L.gsim_graph_destroy(g)
    nb = C.c_void_p()
    assert L.gsim_db_neighbors(t._h, 0.5, 0, 1.0, 1.0, 0, n, C.byref(nb)) == 0
    assert L.gsim_graph_get_knn_stats(nb, C.byref(ks)) == -1 and L.gsim_graph_get_join_stats(nb, C.byref(js)) == -1
    L.gsim_graph_destroy(nb)
    want = t.knn(k, TINY)
    t.close()
    fdb = FingerprintDB(1024, n, "k", [db], [b"s%d" % i for i in range(n)], [b"i%d" % i for i in range(n)])
    fdb.copyToGPU()
    assert as_bytes(fdb.knn(k, TINY)) == as_bytes(want)


def test_the_search_state_is_left_as_it_was():
    n, W, k = 3000, 32, 16
    db = O.synth_rows(0xC0B, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    t.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 1500, 2999]])

    def searches():
        hits, approx = t.search(q, 50, 0.4)
        bufs = (np.zeros((len(q), 50), capi.HIT_DTYPE), np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint64))
        t.search_each_into(q, 50, bufs, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes() + b"".join(bufs[0][i, :bufs[1][i]].tobytes() for i in range(len(q))) + bufs[2].tobytes()

    before = searches()
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0 = t.timing()
    got = t.knn(k, TINY)
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    with pytest.raises(capi.GsimError) as e:
        t.knn(0, TINY)  # a failed call ...
    assert e.value.code == -1
    again = t.knn(k, TINY)  # ... and a correct one right after it
    assert as_bytes(again) == as_bytes(got)
    assert searches() == before
    rows = list(range(0, n, 29))
    want = expected(db, k, TINY, rows=rows)
    for x, i in enumerate(rows):
        a, b = int(got[0][i]), int(got[0][i + 1])
        assert np.array_equal(got[1][a:b], want[1][int(want[0][x]):int(want[0][x + 1])]), i
    t.close()


def test_generated_and_attached_tables():
    import torch
    n, W, k, seed = 2500, 5, 7, 0xC0C
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    want = expected(db, k, TINY)
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    same(g.knn(k, TINY), want, "generated")
    g.close()
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), n, 0)
    same(a.knn(k, TINY), want, "attached (160 bits: a zero-padded copy)")
    same(a.knn(k, TINY, row_begin=700, row_end=2222), expected(db, k, TINY, rows=range(700, 2222)), "attached, a range")
    a.close()
    del ten


def test_a_long_table():
    """1 M x 1024-bit Morgan rows, owners [500000, 500512), k = 16: 5 x 10^8 pairs under the default launch plan, thousands of column
    tiles.  Every list equals Table.search(row, 17) minus the row."""
    n, seed, k, lo, hi = 1_000_000, 0xC0FFEE, 16, 500_000, 500_512
    t = capi.Table(1024).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    st = {}
    indptr, indices, scores = t.knn(k, TINY, row_begin=lo, row_end=hi, stats=st)
    assert st["pairs"] == 512 * 10**6 and st["rows"] == 512 and st["launches"] > 1, st
    q = np.stack([capi.synth_row(seed, capi.SYNTH_MORGAN, r, 1024) for r in range(lo, hi)])
    hits, _ = t.search(q, k + 1, TINY)
    t.close()
    full = 0
    for x, r in enumerate(range(lo, hi)):
        h = hits[x][hits[x]["row"] != r][:k]
        a, b = int(indptr[x]), int(indptr[x + 1])
        assert np.array_equal(indices[a:b], h["row"]), r
        assert np.array_equal(scores[a:b].view(np.uint32), h["score"].view(np.uint32)), r
        full += b - a == k
    assert full >= 500
    print("long table:", st)


def test_twice():
    n, W, k = 1200, 32, 32
    db = planted(0xC0D, O.KIND_MORGAN, n, W)
    t = table(db)
    a = t.knn(k, TINY)
    b = t.knn(k, TINY)
    assert as_bytes(a) == as_bytes(b)
    same(a, expected(db, k, TINY), "twice")
    t.close()
