"""Exact k-nearest-neighbour joins on the GPU (gsim_db_knn_join / gsim_db_knn_queries).

Expected values: list i = oracle_lib.search(left row i, table, k, cutoff, ...) -- the rule's first sentence (include/gpusim_hip.h).
Indices are compared exactly and scores by their bits: no tolerances anywhere.  One search at k + 1 = 129 per left row and metric
gives every expected list of a table (the first k hits: search's order is total) and the candidate behind each.

The parity tables are test_gpu_knn.py's kinds and widths, n = 1200 table rows (700 dense): five column tiles of 256 rows (three),
the last of 176 (188).  GSIM_KNN_JOIN_SEGMENTS = 5 cuts the 1200-row tables into the segments [0, 256), [256, 512), [512, 768),
[768, 1024), [1024, 1200); on the 700-row tables it is clamped to their three tiles: [0, 256), [256, 512), [512, 700).  Planted,
so that the conditions below hold by construction:
  * fingerprint F (synthetic row 5) at table rows 5, 300, 310, 600, 900, 1190 (700 rows: 5, 300, 310, 400, 500, 600): every
    segment has one, one segment has more; seven left rows equal F.  At k = 1 and k = 5 their lists are cut inside the 1.0 tie
    group, between copies that lie in different segments (k = 1: rows 5 | 300; k = 5: rows 900 | 1190, or 500 | 600);
  * fingerprint G (synthetic row 7) at the 128 table rows 11, 14, ... 392 and at rows n - 60 and n - 59; seven left rows equal G.
    At k = 128 their lists are the 128 copies up to row 392 (second segment), cut in front of row n - 60 (last segment);
  * an all-zero left row (150) and an all-zero table row (n / 2 + 1).
Non-vacuity, asserted on the EXPECTED result of every compared (table, metric, k) with all 300 left rows: at least 5 full lists
whose k-th and (k + 1)-th candidates score the same and lie in different segments of the S = 5 cut -- so the merge's tie rule
decides them -- and exactly the all-zero left row's list empty (fewest such lists, counted on the CPU with the oracle: 7, the
planted ones).  The left rows are the 300 rows that follow the table's in the same synthetic library (a library of its own has
nothing near the table at a biting cutoff).  The left sizes 1, 63 and 65 are the first rows of the same left table (row 0 is a
copy of F, row 1 of G); 300 is one full owner tile and one of 44 rows, a single wave of 44 lanes.

Biting cutoffs (k = 5, 300 left rows; counted on the CPU with the oracle): non-empty lists shorter than k -- sparse 128-bit at 0.3
Tanimoto 96, at 0.5 Tversky 49; Morgan 128-bit at 0.5 92; Morgan 1024-bit at 0.3 11; Morgan 2048-bit at 0.3 Tversky 16; Morgan
4096-bit at 0.3 Tversky 29.  (Morgan 2048- and 4096-bit rows under Tanimoto at 0.3 have 3 such lists each among these left rows and
none at 0.5: too few for the condition, so the wide tables are cut under Tversky.)  Asserted >= 5 each."""
import contextlib
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from gpusimilarity_amd.fingerprintdb import FingerprintDB

pytestmark = pytest.mark.gpu
NT = 16
SEGS, PAIRS = "GSIM_KNN_JOIN_SEGMENTS", "GSIM_KNN_JOIN_LAUNCH_PAIRS"
TINY = float(np.nextafter(np.float32(0), np.float32(1)))  # the smallest positive float: "every row with a non-zero score"
TAN = dict()
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
COL_TILE = 256
NL = 300
F_LEFT = [0, 10, 20, 64, 100, 200, 299]
G_LEFT = [1, 11, 21, 65, 101, 201, 298]
ZERO_LEFT = 150


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


def table(db, segments=None, pairs=None, base=0):
    with knobs(**{SEGS: segments, PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def seg_of(row, n, S=5):
    """the segment of a table row under GSIM_KNN_JOIN_SEGMENTS = S (clamped to the column tiles), as gsim::knn_join_seg_begin cuts"""
    nct = -(-n // COL_TILE)
    S = min(S, nct)
    begins = [min(-(-s * nct // S) * COL_TILE, n) for s in range(S + 1)]
    return int(np.searchsorted(begins, row, side="right")) - 1


def f_rows(n):
    return [5, 300, 310, 600, 900, 1190] if n == 1200 else [5, 300, 310, 400, 500, 600]


def g_rows(n):
    return list(range(11, 11 + 3 * 128, 3)) + [n - 60, n - 59]


def planted(seed, kind, n, W):
    """-> (table rows, left rows)"""
    db = O.synth_rows(seed, kind, 0, n, W)
    F, G = db[5].copy(), db[7].copy()
    db[f_rows(n)] = F
    db[g_rows(n)] = G
    db[n // 2 + 1] = 0
    left = O.synth_rows(seed, kind, n, NL, W)  # the next rows of the same synthetic library
    left[F_LEFT] = F
    left[G_LEFT] = G
    left[ZERO_LEFT] = 0
    return db, left


def oracle_hits(left, db, k, cutoff, kw=TAN):
    """left row i -> the hits of oracle_lib.search(left row i, table, k, cutoff, ...)"""
    def one(q):
        return O.search(q, db, k, cutoff, kw.get("metric", O.METRIC_TANIMOTO), kw.get("alpha", 1.0), kw.get("beta", 1.0))[0]
    with ThreadPoolExecutor(NT) as pool:
        return list(pool.map(one, left))


def csr_of(hits, k, base=0):
    lists = [h[:k] for h in hits]
    indptr = np.zeros(len(lists) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(h) for h in lists])
    cat = np.concatenate(lists) if lists else np.zeros(0, O.HIT_DTYPE)
    return indptr, cat["row"].astype(np.uint32) + np.uint32(base), cat["score"].astype(np.float32)


def expected(left, db, k, cutoff, kw=TAN, base=0):
    return csr_of(oracle_hits(left, db, k, cutoff, kw), k, base)


def counts(csr):
    return np.diff(csr[0].astype(np.int64))


def split_ties(hits, k, n):
    """full lists whose k-th and (k + 1)-th candidates (hits: a search at k + 1 or more) score the same and lie in different segments"""
    return sum(1 for h in hits if len(h) > k and h["score"][k] == h["score"][k - 1] and seg_of(h["row"][k], n) != seg_of(h["row"][k - 1], n))


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indptr")
    assert np.array_equal(got[1], want[1]), (what, "indices")
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (what, "scores")


def as_bytes(csr):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in csr)


def test_the_segment_cut_of_this_file_is_the_one_described():
    assert [seg_of(r, 1200) for r in f_rows(1200)] == [0, 1, 1, 2, 3, 4] and [seg_of(r, 700) for r in f_rows(700)] == [0, 1, 1, 1, 1, 2]
    assert seg_of(392, 1200) == 1 and seg_of(1140, 1200) == 4 and seg_of(392, 700) == 1 and seg_of(640, 700) == 2
    assert [seg_of(r, 1200) for r in (255, 256, 1023, 1024, 1199)] == [0, 1, 3, 4, 4]
    assert not set(f_rows(1200)) & set(g_rows(1200)) and not set(f_rows(700)) & set(g_rows(700))
    assert 601 not in f_rows(1200) + g_rows(1200) and 351 not in f_rows(700) + g_rows(700)


WIDTHS = [128, 160, 256, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    """n = 1200 (700 dense); nl = 1, 63, 65, 300; k = 1, 5, 128; Tanimoto and Tversky 0.5 / 0.5; 1, 2 and 5 segments."""
    W = bits // 32
    n = 1200 if kind != O.KIND_DENSE else 700
    db, left = planted(0xBE11 + bits + 7 * kind, kind, n, W)
    tables = {S: table(db, segments=S) for S in (1, 2, 5)}
    lt = table(left)
    for kw in (TAN, TV):
        hits = oracle_hits(left, db, 129, TINY, kw)
        for k in (1, 5, 128):
            what = (bits, kind, kw, k)
            want = csr_of(hits, k)
            cuts = split_ties(hits, k, n)
            empty = np.flatnonzero(counts(want) == 0)
            print(what, "full", int((counts(want) == k).sum()), "ties cut between segments", cuts, "empty", empty.tolist())
            assert cuts >= 5 and empty.tolist() == [ZERO_LEFT], what
            for nl in (1, 63, 65, NL):
                part = csr_of(hits[:nl], k)
                for S, t in tables.items():
                    st = {}
                    got = t.knn_join(lt, k, TINY, row_end=nl, stats=st, **kw)
                    same(got, part, what + (nl, S))
                    assert st["left_rows"] == nl and st["table_rows"] == n and st["pairs"] == nl * n and st["entries"] == len(got[1]), st
                    assert st["segments"] == min(S, -(-n // COL_TILE)) and st["merge_launches"] == (S > 1) and st["fold_launches"] >= 1, st
                    assert st["inserts"] >= st["partial_entries"] >= st["entries"], st
    for t in tables.values():
        t.close()
    lt.close()


BITING = [(128, O.KIND_SPARSE, TAN, 0.3), (128, O.KIND_SPARSE, TV, 0.5), (128, O.KIND_MORGAN, TAN, 0.5), (1024, O.KIND_MORGAN, TAN, 0.3),
          (2048, O.KIND_MORGAN, TV, 0.3), (4096, O.KIND_MORGAN, TV, 0.3)]


@pytest.mark.parametrize("bits,kind,kw,cutoff", BITING)
def test_parity_with_a_biting_cutoff(bits, kind, kw, cutoff):
    n, k = 1200, 5
    db, left = planted(0xBE11 + bits + 7 * kind, kind, n, bits // 32)
    want = expected(left, db, k, cutoff, kw)
    c = counts(want)
    print(bits, kind, kw, cutoff, "full", int((c == k).sum()), "short", int(((c > 0) & (c < k)).sum()), "empty", int((c == 0).sum()))
    assert int(((c > 0) & (c < k)).sum()) >= 5, (bits, kind, kw)
    for S in (1, 5):
        t = table(db, segments=S)
        same(t.knn_join(left, k, cutoff, **kw), want, (bits, kind, kw, cutoff, S))
        t.close()


@pytest.mark.parametrize("bits", [1024, 256])
def test_asymmetric_tversky(bits):
    """The left row is the query: a = popc(left row) takes alpha, b = popc(table row) takes beta."""
    n, k = 1200, 5
    db, left = planted(0xA5E + bits, O.KIND_MORGAN, n, bits // 32)
    tables = [table(db, segments=S) for S in (1, 5)]
    for alpha, beta in ((0.3, 0.7), (1.0, 0.0)):
        kw = dict(metric=capi.METRIC_TVERSKY, alpha=alpha, beta=beta)
        hits = oracle_hits(left, db, k + 1, TINY, kw)
        want = csr_of(hits, k)
        flipped = expected(left, db, k, TINY, dict(kw, alpha=beta, beta=alpha))
        assert split_ties(hits, k, n) >= 5 and np.flatnonzero(counts(want) == 0).tolist() == [ZERO_LEFT]
        assert not np.array_equal(want[1], flipped[1]), "the weights' roles matter on this table"
        for t in tables:
            same(t.knn_join(left, k, TINY, **kw), want, (bits, alpha, beta))
    for t in tables:
        t.close()


def test_fewer_table_rows_than_k():
    W = 32
    left = O.synth_rows(0xFE4, O.KIND_MORGAN, 0, 70, W)
    for n in (1, 2, 40, 65, 257):
        db = O.synth_rows(0xFE3 + n, O.KIND_MORGAN, 0, n, W)
        if n == 40:
            db[20] = 0  # (in nobody's list: 39 rows at the most)
        want = expected(left, db, 128, TINY)
        assert counts(want).max() == (min(n, 128) if n != 40 else 39) and int((counts(want) == counts(want).max()).sum()) >= 5
        for S in (1, 5):
            t = table(db, segments=S)
            st = {}
            got = t.knn_join(left, 128, TINY, stats=st)
            same(got, want, (n, S))
            assert st["segments"] == min(S, -(-n // COL_TILE)) and len(got[0]) == 71
            t.close()


def test_cutoffs_equal_to_scores_that_occur():
    """cutoff 0.5 with c / (a + b - c) = 1/2 pairs present: they are listed (>=); RN(1/3) pairs at cutoff RN(1/3)."""
    n, W, k = 900, 32, 5
    db = O.synth_rows(0x7133, O.KIND_SPARSE, 0, n, W)
    left = O.synth_rows(0x7134, O.KIND_SPARSE, 0, 70, W)

    def bits(*ranges):
        x = np.zeros(W * 32, np.uint8)
        for lo, hi in ranges:
            x[lo:hi] = 1
        return np.packbits(x, bitorder="little").view(np.uint32)

    left[3] = bits((0, 40))            # 40 bits
    db[700] = bits((0, 20))            # vs left 3: c = 20, a + b - c = 40: exactly 1/2
    left[66] = bits((0, 20))
    db[12] = bits((0, 10), (40, 50))   # vs left 66: c = 10, a + b - c = 30: RN(1/3)
    tables = [table(db, segments=S) for S in (1, 3)]
    for cutoff in (np.float32(0.5), np.float32(1.0) / np.float32(3.0)):
        want = expected(left, db, k, float(cutoff))
        assert (want[2] == cutoff).any() and len(want[1]) >= 2, cutoff
        above = float(np.nextafter(cutoff, np.float32(2)))
        fewer = expected(left, db, k, above)
        assert len(fewer[1]) < len(want[1])
        for t in tables:
            same(t.knn_join(left, k, float(cutoff)), want, cutoff)
            same(t.knn_join(left, k, above), fewer, above)
    for t in tables:
        t.close()


@pytest.fixture(scope="module")
def morgan():
    """One planted 1200 x 1024-bit Morgan table with its left rows and the expected lists at k = 5 and 128 (left unchanged by the tests)."""
    n, W = 1200, 32
    db, left = planted(0xC07, O.KIND_MORGAN, n, W)
    hits = oracle_hits(left, db, 129, TINY)
    return dict(n=n, W=W, db=db, left=left, hits=hits, k5=csr_of(hits, 5), k128=csr_of(hits, 128))


def test_no_left_rows(morgan):
    t, lt = table(morgan["db"]), table(morgan["left"])
    for got in (t.knn_join(lt, 5, TINY, row_begin=17, row_end=17), t.knn_join(np.zeros((0, morgan["W"]), np.uint32), 5, TINY),
                t.knn_join(t, 5, TINY, row_begin=9, row_end=9, exclude_self=True)):
        assert got[0].tolist() == [0] and len(got[1]) == 0 and len(got[2]) == 0
    st = {}
    t.knn_join(lt, 5, TINY, row_begin=300, row_end=300, stats=st)
    assert st["left_rows"] == 0 and st["pairs"] == 0 and st["entries"] == 0 and st["fold_launches"] == 0
    t.close()
    lt.close()


def test_the_result_depends_on_neither_knob(morgan):
    n, db, left = morgan["n"], morgan["db"], morgan["left"]
    ntiles = -(-n // COL_TILE)
    ref = table(db, segments=1)
    st0 = {}
    a = ref.knn_join(left, 5, TINY, stats=st0)
    same(a, morgan["k5"], "one segment, default plan")
    big = ref.knn_join(left, 128, TINY, **TV)
    ref.close()
    assert st0["segments"] == 1 and st0["merge_launches"] == 0 and st0["partial_entries"] == st0["entries"]
    for S, want_S in ((1, 1), (2, 2), (3, 3), (5, 5), (99, ntiles)):
        t = table(db, segments=S)
        st = {}
        b = t.knn_join(left, 5, TINY, stats=st)
        assert st["segments"] == want_S and st["merge_launches"] == (want_S > 1), (S, st)
        assert as_bytes(b) == as_bytes(a), S
        assert st["pairs"] == st0["pairs"] == NL * n and st["entries"] == st0["entries"] and st["partial_entries"] >= st["entries"]
        assert as_bytes(t.knn_join(left, 128, TINY, **TV)) == as_bytes(big), S
        t.close()
    # a launch never covers less than one column tile per segment: pairs = 1 gives the longest segment's tiles as launches
    seen = set()
    for S, pairs, launches in ((1, 1, ntiles), (1, NL * 2 * COL_TILE, -(-ntiles // 2)), (2, 1, 3), (2, NL * 2 * 2 * COL_TILE, 2), (5, 1, 1)):
        t = table(db, segments=S, pairs=pairs)
        st = {}
        b = t.knn_join(left, 5, TINY, stats=st)
        assert st["fold_launches"] == launches, (S, pairs, st)
        assert as_bytes(b) == as_bytes(a), (S, pairs)
        assert as_bytes(t.knn_join(left, 128, TINY, **TV)) == as_bytes(big), (S, pairs)
        seen.add(st["fold_launches"])
        t.close()
    assert len(seen) >= 4 and st0["fold_launches"] == 1


def test_a_handle_and_host_queries_give_the_same_bytes(morgan):
    db, left = morgan["db"], morgan["left"]
    lt = table(left, base=5000)  # (the left handle's row base plays no part)
    for S in (1, 5):
        t = table(db, segments=S)
        a = t.knn_join(lt, 128, TINY)
        b = t.knn_join(left, 128, TINY)
        same(a, morgan["k128"], S)
        assert as_bytes(a) == as_bytes(b), S
        assert as_bytes(t.knn_join(lt, 5, 0.3, row_begin=60, row_end=70)) == as_bytes(t.knn_join(left[60:70], 5, 0.3)), S
        t.close()
    lt.close()


def test_left_ranges_and_the_row_bases(morgan):
    n, db, left, k, base = morgan["n"], morgan["db"], morgan["left"], 5, 1000
    lt = table(left)
    for S in (1, 5):
        t = table(db, segments=S)
        full = t.knn_join(lt, k, TINY)
        same(full, morgan["k5"], "full")
        ind, sc = [], []
        for lo, hi in ((0, 100), (100, 101), (101, NL)):
            st = {}
            p_indptr, p_ind, p_sc = t.knn_join(lt, k, TINY, row_begin=lo, row_end=hi, stats=st)
            assert len(p_indptr) == hi - lo + 1 and st["left_rows"] == hi - lo and st["pairs"] == (hi - lo) * n
            assert np.array_equal(p_indptr.astype(np.int64), full[0][lo:hi + 1].astype(np.int64) - int(full[0][lo]))
            ind.append(p_ind)
            sc.append(p_sc)
        assert np.array_equal(np.concatenate(ind), full[1])
        assert np.array_equal(np.concatenate(sc).view(np.uint32), full[2].view(np.uint32))
        # the table's base is added, the left's is ignored
        t.set_row_base(base)
        lt.set_row_base(77777)
        based = t.knn_join(lt, k, TINY)
        assert np.array_equal(based[0], full[0]) and np.array_equal(based[1], full[1] + np.uint32(base))
        assert np.array_equal(based[2].view(np.uint32), full[2].view(np.uint32))
        same(based, csr_of(morgan["hits"], k, base), "based")
        part = t.knn_join(lt, k, TINY, row_begin=199, row_end=250)
        assert np.array_equal(part[1], full[1][int(full[0][199]):int(full[0][250])] + np.uint32(base))
        lt.set_row_base(0)
        t.close()
    lt.close()


def test_the_table_against_itself(morgan):
    """left == db.  Without the flag every non-zero row's list starts at 1.0 with itself or its lowest-numbered duplicate; with
    GSIM_KNN_EXCLUDE_SELF the result is gsim_db_knn's, byte for byte, on full and partial ranges."""
    n, db = morgan["n"], morgan["db"]
    lowest = {}
    for r in range(n):
        lowest.setdefault(db[r].tobytes(), r)
    want = {k: expected(db, db, k, TINY) for k in (1, 5)}
    for S in (1, 5):
        t = table(db, segments=S)
        for k in (1, 5):
            got = t.knn_join(t, k, TINY)
            same(got, want[k], ("left == db", S, k))
            for r in range(n):
                a, b = int(got[0][r]), int(got[0][r + 1])
                if r == n // 2 + 1:
                    assert a == b
                else:
                    assert got[1][a] == lowest[db[r].tobytes()] and got[2][a] == 1.0, r
        for k, kw in ((1, TAN), (5, TAN), (128, TV)):
            for lo, hi in ((0, n), (0, 1), (299, 301), (5, 700), (1024, n)):
                a = t.knn_join(t, k, TINY, row_begin=lo, row_end=hi, exclude_self=True, **kw)
                b = t.knn(k, TINY, row_begin=lo, row_end=hi, **kw)
                assert as_bytes(a) == as_bytes(b), (S, k, lo, hi)
        a = t.knn_join(t, 5, 0.3, exclude_self=True)
        assert as_bytes(a) == as_bytes(t.knn(5, 0.3)) and 0 < len(a[1]) < 5 * n
        t.close()


def test_against_search_on_the_gpu(morgan):
    """Every list = Table.search(left row, 128) on the same table, hit for hit."""
    db, left = morgan["db"], morgan["left"]
    for S in (1, 5):
        t = table(db, segments=S)
        got = t.knn_join(left, 128, TINY)
        full = 0
        for lo in range(0, NL, 100):
            hits, _ = t.search(np.ascontiguousarray(left[lo:lo + 100]), 128, TINY)
            for x, h in enumerate(hits):
                a, b = int(got[0][lo + x]), int(got[0][lo + x + 1])
                assert np.array_equal(got[1][a:b], h["row"]), (S, lo + x)
                assert np.array_equal(got[2][a:b].view(np.uint32), h["score"].view(np.uint32)), (S, lo + x)
                full += b - a == 128
        assert full >= 250
        t.close()


def test_against_the_threshold_join(morgan):
    """Every list = the first k entries of that left row's gsim_db_join list in JOIN_BY_SCORE order, at a cutoff that bites."""
    db, left, k, cutoff = morgan["db"], morgan["left"], 5, 0.3
    for S in (1, 5):
        t = table(db, segments=S)
        indptr, indices, scores = t.join(left, cutoff, order=capi.JOIN_BY_SCORE)
        got = t.knn_join(left, k, cutoff)
        t.close()
        short = 0
        for i in range(NL):
            lo, hi = int(indptr[i]), int(indptr[i + 1])
            a, b = int(got[0][i]), int(got[0][i + 1])
            assert b - a == min(k, hi - lo), i
            hi = min(hi, lo + k)
            assert np.array_equal(got[1][a:b], indices[lo:hi]) and np.array_equal(got[2][a:b].view(np.uint32), scores[lo:hi].view(np.uint32)), i
            short += 0 < b - a < k
        assert short >= 5


def test_the_search_state_of_both_handles_is_left_as_it_was():
    n, W, k = 3000, 32, 16
    db = O.synth_rows(0xC0B, O.KIND_MORGAN, 0, n, W)
    left = O.synth_rows(0xC1B, O.KIND_MORGAN, 0, 700, W)
    t, lt = table(db, segments=4), table(left)
    t.enable_timing(True)
    lt.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 1500, 2999]])

    def searches(x):
        hits, approx = x.search(q, 50, 0.4)
        bufs = (np.zeros((len(q), 50), capi.HIT_DTYPE), np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint64))
        x.search_each_into(q, 50, bufs, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes() + b"".join(bufs[0][i, :bufs[1][i]].tobytes() for i in range(len(q))) + bufs[2].tobytes()

    before = searches(t), searches(lt)
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0, l0 = t.timing(), lt.timing()
    got = t.knn_join(lt, k, TINY)
    t1, l1 = t.timing(), lt.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters] and [l0[c] for c in counters] == [l1[c] for c in counters]
    assert (searches(t), searches(lt)) == before
    with pytest.raises(capi.GsimError) as e:
        t.knn_join(lt, 0, TINY)  # a failed call ...
    assert e.value.code == -1
    again = t.knn_join(lt, k, TINY)  # ... and a correct one right after it
    assert as_bytes(again) == as_bytes(got)
    assert (searches(t), searches(lt)) == before
    same(got, expected(left, db, k, TINY), "3000 x 700")
    t.close()
    lt.close()


def test_generated_and_attached_tables_on_either_side():
    import torch
    n, nl, W, k, seed, lseed = 2500, 400, 5, 7, 0xC0C, 0xC1C
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    left = O.synth_rows(lseed, O.KIND_MORGAN, 0, nl, W)
    want = expected(left, db, k, TINY)
    with knobs(**{SEGS: 3}):
        g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
        gl = capi.Table(W * 32).generate(lseed, capi.SYNTH_MORGAN, 0, nl, 0)
        a, al = capi.Table(W * 32), capi.Table(W * 32)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    lten = torch.from_numpy(left.view(np.int32).copy()).to("cuda:0")
    a.attach_device_rows(ten.data_ptr(), n, 0)
    al.attach_device_rows(lten.data_ptr(), nl, 0)
    same(g.knn_join(gl, k, TINY), want, "generated x generated")
    same(g.knn_join(al, k, TINY), want, "generated x attached (160 bits: zero-padded copies)")
    same(a.knn_join(gl, k, TINY), want, "attached x generated")
    same(a.knn_join(al, k, TINY), want, "attached x attached")
    part = a.knn_join(al, k, TINY, row_begin=70, row_end=333)
    assert np.array_equal(part[1], want[1][int(want[0][70]):int(want[0][333])])
    assert as_bytes(a.knn_join(a, k, TINY, row_begin=700, row_end=2222, exclude_self=True)) == as_bytes(a.knn(k, TINY, row_begin=700, row_end=2222))
    for x in (g, gl, a, al):
        x.close()
    del ten, lten


def test_the_graph_object_and_the_wrapper(morgan):
    """The result is a gsim_graph of its own kind: the other accessors refuse it and its accessor refuses theirs."""
    n, db, left, k = morgan["n"], morgan["db"], morgan["left"], 5
    t, lt = table(db, segments=5), table(left)
    L = capi.load()
    g = C.c_void_p()
    assert L.gsim_db_knn_join(t._h, lt._h, 0, NL, k, TINY, 0, 1.0, 1.0, 0, C.byref(g)) == 0 and g.value
    js, gs, ks, kj = capi.GsimJoinStats(), capi.GsimGraphStats(), capi.GsimKnnStats(), capi.GsimKnnJoinStats()
    assert L.gsim_graph_get_join_stats(g, C.byref(js)) == -1 and L.gsim_graph_get_knn_stats(g, C.byref(ks)) == -1
    assert L.gsim_graph_get_stats(g, C.byref(gs)) == 0 and L.gsim_graph_get_knn_join_stats(g, C.byref(kj)) == 0
    rows, nnz = C.c_uint64(0), C.c_uint64(0)
    assert L.gsim_graph_shape(g, C.byref(rows), C.byref(nnz)) == 0 and rows.value == NL
    assert gs.launches == kj.fold_launches + kj.merge_launches == 2 and gs.pairs == kj.entries == nnz.value
    assert kj.left_rows == NL and kj.table_rows == n and kj.pairs == NL * n and kj.segments == 5 and kj.partial_entries >= kj.entries
    assert kj.kernel_ms > 0 and kj.merge_ms > 0 and kj.wall_ms > 0 and kj.clock_mhz > 100
    L.gsim_graph_destroy(g)
    q = np.ascontiguousarray(left[:9])
    assert L.gsim_db_knn_queries(t._h, q.ctypes.data_as(C.POINTER(C.c_uint32)), 9, k, TINY, 0, 1.0, 1.0, C.byref(g)) == 0
    assert L.gsim_graph_get_knn_join_stats(g, C.byref(kj)) == 0 and kj.left_rows == 9 and L.gsim_graph_get_knn_stats(g, C.byref(ks)) == -1
    L.gsim_graph_destroy(g)
    for make in (lambda o: L.gsim_db_neighbors(t._h, 0.5, 0, 1.0, 1.0, 0, n, o), lambda o: L.gsim_db_knn(t._h, k, TINY, 0, 1.0, 1.0, 0, n, o),
                 lambda o: L.gsim_db_join(t._h, lt._h, 0, NL, 0.5, 0, 1.0, 1.0, 0, o)):
        other = C.c_void_p()
        assert make(C.byref(other)) == 0
        assert L.gsim_graph_get_knn_join_stats(other, C.byref(kj)) == -1 and len(L.gsim_last_error()) > 0
        L.gsim_graph_destroy(other)
    want = t.knn_join(lt, k, TINY)
    same(want, morgan["k5"], "wrapper")
    t.close()
    lt.close()
    fdb = FingerprintDB(1024, n, "k", [db], [b"s%d" % i for i in range(n)], [b"i%d" % i for i in range(n)])
    fdb.copyToGPU()
    fl = FingerprintDB(1024, NL, "l", [left], [b"s%d" % i for i in range(NL)], [b"i%d" % i for i in range(NL)])
    fl.copyToGPU()
    assert as_bytes(fdb.knn_join(fl, k, TINY)) == as_bytes(want) == as_bytes(fdb.knn_join(left, k, TINY))
    assert as_bytes(fdb.knn_join(fdb, k, TINY, exclude_self=True)) == as_bytes(fdb.knn(k, TINY))


def test_twice(morgan):
    t, lt = table(morgan["db"], segments=5), table(morgan["left"])
    a = t.knn_join(lt, 128, TINY)
    b = t.knn_join(lt, 128, TINY)
    assert as_bytes(a) == as_bytes(b)
    same(a, morgan["k128"], "twice")
    t.close()
    lt.close()


def test_a_long_table():
    """512 generated left rows against 1 M x 1024-bit generated Morgan rows, k = 8, the automatic plan: the columns are split (two
    owner tiles on a device of far more than one CU) and 64 sampled lists equal Table.search(left row, 8)."""
    n, nl, seed, lseed, k = 1_000_000, 512, 0xC0FFEE, 0xDECAF, 8
    t = capi.Table(1024).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    lt = capi.Table(1024).generate(lseed, capi.SYNTH_MORGAN, 0, nl, 0)
    st = {}
    indptr, indices, scores = t.knn_join(lt, k, TINY, stats=st)
    assert st["pairs"] == 512 * 10**6 and st["left_rows"] == 512 and st["segments"] > 1 and st["merge_launches"] == 1, st
    sample = list(range(0, nl, 8))
    q = np.stack([capi.synth_row(lseed, capi.SYNTH_MORGAN, r, 1024) for r in sample])
    hits, _ = t.search(q, k, TINY)
    t.close()
    lt.close()
    assert len(sample) == 64
    for x, r in enumerate(sample):
        a, b = int(indptr[r]), int(indptr[r + 1])
        assert b - a == k and np.array_equal(indices[a:b], hits[x]["row"]), r
        assert np.array_equal(scores[a:b].view(np.uint32), hits[x]["score"].view(np.uint32)), r
    print("long table:", st)
