"""Row sets on the GPU (gsim_rowset_*, gsim_db_search_rows): every result against the oracle run over the selected rows only --
oracle_lib.search(q, db[rows_sorted], k, cutoff, ...) with row = rows_sorted[hit.row] -- hits, counts and approx, both routes
(gather, streaming) forced in turn and compared with each other byte for byte.  Everything is exact: no tolerances."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
NT = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "GSIM_SUBSET_GATHER_MAX_PERMILLE"
STREAM, GATHER = "0", "1000"  # values of the knob that force either route
ROUTES = [STREAM, GATHER]
TAN = dict()
TV37 = dict(metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7)
SCREEN = dict(metric=capi.METRIC_TVERSKY, alpha=1.0, beta=0.0)


@contextlib.contextmanager
def knob(value):
    """The route knob is read once per handle, by gsim_db_create: set it around the creation of a table."""
    old = os.environ.get(KNOB)
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def table(db, route=None, base=0):
    with knob(route):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def generated(seed, kind, n, bits=1024, route=None):
    with knob(route):
        return capi.Table(bits).generate(seed, kind, 0, n, 0)


def bitmap_of(rows, n):
    m = np.zeros(n, np.uint8)
    m[rows] = 1
    return np.packbits(np.concatenate([m, np.zeros((-n) % 32, np.uint8)]), bitorder="little").view(np.uint32)


def expected(q, db, rows_sorted, k, cutoff, kw, base=0):
    """What the header promises: the search over a table of the selected rows only, rows mapped back."""
    if len(rows_sorted) == 0:
        return np.zeros(0, capi.HIT_DTYPE), 0
    hits, approx = O.search(q, db[rows_sorted], k, cutoff, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0), nthreads=NT)
    hits["row"] = rows_sorted[hits["row"]].astype(np.uint32) + np.uint32(base)
    return hits, approx


def same_hits(got, want, what):
    assert len(got) == len(want), what
    assert np.array_equal(got["row"], want["row"]), what
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), what
    assert np.array_equal(got["common"], want["common"]) and np.array_equal(got["popc_db"], want["popc_db"]), what


def check(t, rs, route, queries, db, rows_sorted, k, cutoff, kw, what, base=0, empty_ok=False):
    """One search_rows call against the oracle; returns the raw result for the route-against-route comparison."""
    hits, approx, st = t.search_rows(rs, queries, k, cutoff, stats=True, **kw)
    assert st["selected"] == len(rows_sorted), what
    if len(rows_sorted):
        assert st["queries_gather"] == (len(queries) if route == GATHER else 0), what
        assert st["queries_stream"] == (len(queries) if route == STREAM else 0), what
        assert st["launches"] >= 3 * len(queries) and st["kernel_ms"] > 0 and st["wall_ms"] > 0, what
    for i, q in enumerate(queries):
        want, wap = expected(q, db, rows_sorted, k, cutoff, kw, base)
        print(what, "query", i, "expected hits", len(want), "approx", wap, "got", len(hits[i]), int(approx[i]))
        if empty_ok:
            assert len(want) == 0 and wap == 0, what
        else:
            assert len(want) > 0, ("a vacuous case", what)
        same_hits(hits[i], want, (what, i))
        assert int(approx[i]) == wap, (what, i)
    return b"".join(h.tobytes() for h in hits) + approx.tobytes()


WIDTHS = [128, 160, 256, 416, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


def set_shapes(n, rng):
    zero = n // 2
    chunk_tail = np.arange(n - 3, n)  # inside the table's last partial chunk for every width (n % chunk >= 3 for chunks of 8 ... 512 rows)
    return {
        "random half": np.flatnonzero(rng.random(n) < 0.5),
        "random 2 %": np.flatnonzero(rng.random(n) < 0.02),
        "contiguous range": np.arange(zero - 150, zero + 183),
        "every 64th row": np.arange(5, n, 64),
        "one row": np.array([n // 3]),
        "last partial chunk": chunk_tail,
        "all rows": np.arange(n),
        "empty": np.zeros(0, np.int64),
    }


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    W = bits // 32
    n = 1203 if kind != O.KIND_DENSE else 1190
    assert all(n % c >= 3 for c in (8, 16, 32, 64, 128, 256, 512))
    seed = 0x5B5E7 + bits + 7 * kind
    db = O.synth_rows(seed, kind, 0, n, W)
    zero = n // 2
    db[zero] = 0  # an all-zero row: NaN against an all-zero query, never counted
    rng = np.random.default_rng(bits * 5 + kind)
    tables = {r: table(db, r) for r in ROUTES}
    shapes = set_shapes(n, rng)
    excluded = np.flatnonzero(rng.random(n) < 0.3)
    shapes["exclusion"] = np.setdiff1d(np.arange(n), excluded)
    assert zero in shapes["contiguous range"] and zero in shapes["all rows"]
    for name, rows in shapes.items():
        rows = np.asarray(rows, np.int64)
        # the same set three ways: a shuffled list with duplicates, a bitmap, and (the exclusion set) its complement
        given = np.concatenate([rows, rows[: max(1, len(rows) // 3)]]) if len(rows) else rows
        given = rng.permutation(given).astype(np.uint32)
        sets = {}
        for r, t in tables.items():
            if name == "exclusion":
                sets[r] = t.rowset(rows=rng.permutation(np.concatenate([excluded, excluded[:9]])).astype(np.uint32), exclude=True)
            else:
                sets[r] = t.rowset(rows=given)
        by_bitmap = tables[STREAM].rowset(bitmap=bitmap_of(rows, n)) if name != "exclusion" else tables[STREAM].rowset(
            bitmap=bitmap_of(excluded, n), exclude=True)
        for rs in list(sets.values()) + [by_bitmap]:
            assert rs.count == len(rows), name
            assert np.array_equal(rs.rows(), rows.astype(np.uint32)), name
        if len(rows):
            pool = rows[rows != zero]
            queries = db[pool[rng.integers(0, len(pool), 2)]]  # rows of the set: every cutoff keeps at least themselves
        else:
            queries = db[[3, 700]]
        cases = [(TAN, k, c) for k in (1, 10, 1000, len(rows) + 5) for c in (0.0, 0.3, 0.8)]
        cases += [(TV37, 10, 0.0), (TV37, 1000, 0.3), (SCREEN, 1000, 1.0), (SCREEN, 1, 1.0)]
        for kw, k, cutoff in cases:
            what = (bits, kind, name, kw, k, cutoff)
            raw = [check(tables[r], sets[r], r, queries, db, rows, k, cutoff, kw, what + (r,), empty_ok=len(rows) == 0) for r in ROUTES]
            assert raw[0] == raw[1], ("the routes differ", what)
        raw_b = check(tables[STREAM], by_bitmap, STREAM, queries, db, rows, 10, 0.3, TAN, (bits, kind, name, "bitmap"), empty_ok=len(rows) == 0)
        raw_l = check(tables[STREAM], sets[STREAM], STREAM, queries, db, rows, 10, 0.3, TAN, (bits, kind, name, "list"), empty_ok=len(rows) == 0)
        assert raw_b == raw_l
        # the all-zero query: NaN against the all-zero row (never counted), 0.0 against the others
        if name == "contiguous range":
            for r in ROUTES:
                hits, approx = tables[r].search_rows(sets[r], np.zeros(W, np.uint32), 5, 0.0)
                want, wap = expected(np.zeros(W, np.uint32), db, rows, 5, 0.0, TAN)
                same_hits(hits[0], want, (bits, kind, "zero query", r))
                assert int(approx[0]) == wap == len(rows)
                hits, approx = tables[r].search_rows(sets[r], np.zeros(W, np.uint32), 5, 0.5)
                assert len(hits[0]) == 0 and int(approx[0]) == 0
        for rs in list(sets.values()) + [by_bitmap]:
            rs.close()
    for t in tables.values():
        t.close()


@pytest.mark.parametrize("bits", [128, 160, 1024, 896])
def test_a_set_of_all_rows_equals_search(bits):
    n, W = 5000, bits // 32
    db = O.synth_rows(0xA11 + bits, O.KIND_MORGAN, 0, n, W)
    q = db[[1, 2500, 4999]]
    for r in ROUTES:
        t = table(db, r)
        every = [t.rowset(rows=np.arange(n, dtype=np.uint32)), t.rowset(rows=np.zeros(0, np.uint32), exclude=True),
                 t.rowset(bitmap=np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32))]
        for k, cutoff, kw in ((10, 0.0, TAN), (1000, 0.2, TAN), (n, 0.0, TAN), (n + 7, 0.1, TV37), (64, 0.9, TAN)):
            want = [t.search(q[i], k, cutoff, **kw) for i in range(len(q))]  # one at a time: the single-query routes
            assert len(want[0][0][0]) > 0
            for rs in every:
                assert rs.count == n
                hits, approx = t.search_rows(rs, q, k, cutoff, **kw)
                for i in range(len(q)):
                    assert hits[i].tobytes() == want[i][0][0].tobytes(), (bits, r, k, cutoff, i)
                    assert int(approx[i]) == int(want[i][1][0])
        for rs in every:
            rs.close()
        t.close()


@pytest.mark.parametrize("route", ROUTES)
def test_excluding_the_top_hits_returns_the_next_best(route):
    n, W = 20000, 32
    db = O.synth_rows(0xE8C1, O.KIND_MORGAN, 0, n, W)
    t = table(db, route, base=5_000_000)
    q = db[777]
    first, _ = t.search(q, 50)
    rs = t.rowset(rows=first[0]["row"], exclude=True)  # hit rows go straight in, row base and all
    assert rs.count == n - 50
    nxt, approx = t.search_rows(rs, q, 50)
    both, _ = t.search(q, 100)
    assert nxt[0].tobytes() == both[0][50:].tobytes() and int(approx[0]) == n - 50
    assert not np.intersect1d(nxt[0]["row"], first[0]["row"]).size
    rs.close()
    t.close()


def test_the_seed_trap():
    """2000 near-copies of the query sit in the table and NOT in the set: a threshold seeded from unselected rows lies above
    the set's k-th best and loses hits.  k = 1000 must come back whole and equal to the oracle."""
    n, W, k = 1_000_000, 32, 1000
    db = O.synth_rows_mt(0x5EED7, O.KIND_MORGAN, 0, n, W, NT)
    rng = np.random.default_rng(77)
    q = db[123_456].copy()
    planted = np.sort(rng.choice(n, 2000, replace=False))
    planted = planted[planted != 123_456]
    copies = np.repeat(q[None, :], len(planted), 0)
    flip = rng.integers(0, W * 32, len(planted))
    copies[np.arange(len(planted)), flip // 32] ^= (np.uint32(1) << (flip % 32).astype(np.uint32))  # one bit off each
    db[planted] = copies
    rows = np.setdiff1d(np.arange(n), np.concatenate([planted, [123_456]]))
    want, wap = expected(q, db, rows, k, 0.0, TAN)
    whole, _ = O.search(q, db, k, 0.0, nthreads=NT)
    assert len(want) == k and whole["score"][k - 1] > want["score"][0], "the planted rows outscore the whole set"
    raws = []
    for r in ROUTES + [None]:
        t = table(db, r)
        rs = t.rowset(rows=np.concatenate([planted, [123_456]]).astype(np.uint32), exclude=True)
        assert rs.count == len(rows)
        t.search(q, k)  # (a whole-table search first: whatever it leaves behind must not seed the next call)
        hits, approx = t.search_rows(rs, q, k)
        print("route", r, "hits", len(hits[0]), "of", k)
        assert len(hits[0]) == k
        same_hits(hits[0], want, r)
        assert int(approx[0]) == wap == len(rows)
        raws.append(hits[0].tobytes())
        rs.close()
        t.close()
    assert raws[0] == raws[1] == raws[2]


def test_one_million_rows_generated():
    """1 M x 1024-bit generated tables, Morgan-shaped and sparse; sets of 10 000 and 500 000 random rows; k = 1000 and k = 10 000
    (above the select kernel's 8192); 8 queries; both routes; against the oracle over the selected rows only."""
    n, W = 1_000_000, 32
    for kind, seed in ((capi.SYNTH_MORGAN, 0x20000), (capi.SYNTH_SPARSE, 0x20001)):
        db = O.synth_rows_mt(seed, kind, 0, n, W, NT)
        rng = np.random.default_rng(seed)
        queries = np.stack([capi.synth_row(seed, kind, n + i, 1024) for i in range(8)])
        sets = {m: np.sort(rng.choice(n, m, replace=False)) for m in (10_000, 500_000)}
        raws = {}
        for r in ROUTES:
            t = generated(seed, kind, n, route=r)
            for m, rows in sets.items():
                rs = t.rowset(rows=rng.permutation(rows).astype(np.uint32))
                assert rs.count == m
                for k in (1000, 10_000):
                    what = (kind, m, k, r)
                    raws[what] = check(t, rs, r, queries, db, rows, k, 0.0, TAN, what)
                raws[(kind, m, "cutoff", r)] = check(t, rs, r, queries[:2], db, rows, 10_000, 0.05, TAN, (kind, m, "cutoff", r))
                rs.close()
            t.close()
        for (kd, m, k, r), raw in raws.items():
            assert raw == raws[(kd, m, k, STREAM)], ("the routes differ", kd, m, k)


@pytest.mark.parametrize("route", ROUTES)
def test_ties_at_the_boundary_keep_the_lowest_selected_rows(route):
    n, W = 200_000, 32
    db = O.synth_rows_mt(0x71E5, O.KIND_MORGAN, 0, n, W, NT)
    rng = np.random.default_rng(5)
    rows = np.flatnonzero(rng.random(n) < 0.4)
    q = db[rows[1000]]
    ranked, _ = expected(q, db, rows, 4000, 0.0, TAN)
    sc = ranked["score"]
    # a k whose k-th score's tie group straddles the cut: members on both sides
    cuts = [k for k in range(200, 3900) if sc[k - 1] == sc[k] and sc[k - 2] == sc[k - 1]]
    assert cuts, "no straddled tie group on this table"
    t = table(db, route)
    rs = t.rowset(rows=rows.astype(np.uint32))
    for k in (cuts[0], cuts[len(cuts) // 2], cuts[-1]):
        hits, _ = t.search_rows(rs, q, k)
        want = ranked[:k]
        same_hits(hits[0], want, (route, k))
        group = ranked[ranked["score"] == sc[k - 1]]
        taken = hits[0][hits[0]["score"] == sc[k - 1]]
        assert 0 < len(taken) < len(group) and np.array_equal(taken["row"], np.sort(group["row"])[: len(taken)])
    rs.close()
    t.close()


@pytest.mark.parametrize("route", ROUTES)
def test_the_search_state_survives(route):
    n, W = 300_000, 32
    with knob(route):
        t = capi.Table(1024).generate(0x57A7E, capi.SYNTH_MORGAN, 0, n, 0)
    t.enable_timing(True)
    q = np.stack([capi.synth_row(0x57A7E, capi.SYNTH_MORGAN, n + i, 1024) for i in range(6)])
    rng = np.random.default_rng(9)
    rs = t.rowset(rows=rng.choice(n, 30_000, replace=False).astype(np.uint32))

    def snapshot():
        out = []
        for k, cutoff in ((100, 0.0), (3000, 0.0), (10_000, 0.1)):
            one = [t.search(q[i], k, cutoff) for i in range(3)]
            bufs = t.make_search_buffers(len(q), k)
            t.search_each_into(q, k, bufs, cutoff)
            out.append(b"".join(h[0][0].tobytes() + h[1].tobytes() for h in one) + b"".join(b.tobytes() for b in bufs))
        return out

    before = snapshot()
    counters = ("handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "backoff_skips", "lane_queries")
    tm0 = t.timing()
    for k, cutoff in ((50, 0.0), (9000, 0.0), (500, 0.2)):
        hits, approx, st = t.search_rows(rs, q, k, cutoff, stats=True)
        assert len(hits[0]) > 0
        assert (st["queries_gather"], st["queries_stream"]) == ((6, 0) if route == GATHER else (0, 6))
    tm1 = t.timing()
    assert {c: tm0[c] for c in counters} == {c: tm1[c] for c in counters}
    mid = snapshot()
    t.search_rows(rs, q[:1], 9000, 0.0)
    after = snapshot()
    assert before == mid == after
    rs.close()
    t.close()


def test_row_base_foreign_sets_and_error_codes():
    n, W, base = 4000, 32, 3_000_000
    db = O.synth_rows(0xBA5E, O.KIND_SPARSE, 0, n, W)
    rows = np.arange(100, 900, 3)
    for r in ROUTES:
        t = table(db, r, base=base)
        rs = t.rowset(rows=(rows + base).astype(np.uint32))
        assert np.array_equal(rs.rows(), (rows + base).astype(np.uint32))
        check(t, rs, r, db[[100, 103]], db, rows, 20, 0.0, TAN, ("row base", r), base=base)
        with pytest.raises(capi.GsimError) as e:
            t.rowset(rows=rows.astype(np.uint32))  # without the base: outside the table
        assert e.value.code == -1
        other = table(db, r)
        with pytest.raises(capi.GsimError) as e:
            other.search_rows(rs, db[0], 5)
        assert e.value.code == -1 and "another handle" in str(e.value)
        rs.close()
        other.close()
        t.close()
    # the default knob names the route that ran: a sparse set gathers, a dense one streams
    t = table(db)
    sparse, dense = t.rowset(rows=np.arange(0, n, 100, dtype=np.uint32)), t.rowset(rows=np.arange(0, n - 1, dtype=np.uint32))
    assert t.search_rows(sparse, db[0], 5, stats=True)[2]["queries_gather"] == 1
    assert t.search_rows(dense, db[0], 5, stats=True)[2]["queries_stream"] == 1
    sparse.close()
    dense.close()
    t.close()
    # a folded table
    f = capi.Table(1024).add_rows(db).set_fold_factor(2).finalize(0, 1)
    with pytest.raises(capi.GsimError) as e:
        f.rowset(rows=np.array([1, 2], np.uint32))
    assert e.value.code == -5
    f.close()
    # a multi-shard handle: two logical devices on one GPU (the test-hooks build of the library)
    from conftest import hooks_env, HOOKS_LIB
    assert os.path.exists(HOOKS_LIB)
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from gpusimilarity_amd import capi\n"
            "t = capi.Table(1024).add_rows(np.ones((512, 32), np.uint32)).finalize(0, 2)\n"
            "u = capi.Table(1024).add_rows(np.ones((512, 32), np.uint32)).finalize(0, 1)\n"
            "assert t.shard_count() == 2\n"
            "rs = u.rowset(rows=np.arange(9, dtype=np.uint32))\n"
            "for f in (lambda: t.rowset(rows=np.arange(9, dtype=np.uint32)), lambda: t.rowset(bitmap=np.ones(16, np.uint32)),\n"
            "          lambda: t.search_rows(rs, np.ones(32, np.uint32), 5)):\n"
            "    try:\n        f()\n    except capi.GsimError as e:\n        print('code', e.code)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=hooks_env(GSIM_TEST_ALIAS_DEVICES="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("code -5") == 2 and r.stdout.count("code -1") == 1, r.stdout + r.stderr
