"""Similarity histograms and hit counts on the GPU (gsim_db_histogram, gsim_db_histogram_queries).

Expected values: for left row i the oracle's scores of row i against every table row (oracle_lib.search with k = N at cutoff 0, as
test_gpu_knn.py does: every row comes back, NaN as 0.0 -- both are bin 0), binned with np.searchsorted(edges_f32, scores_f32,
side="right") and counted.  Counters are compared exactly: no tolerances anywhere.

The parity tables are test_gpu_knn.py's planted tables (the same seeds, seven identical rows, one all-zero row).  Edges are taken
from the data so that boundaries bite: five distinct non-zero values among the oracle's own scores for that table (quantiles of
the distinct values below 1) plus 1.0.  Asserted on the EXPECTED result before anything is compared: every edge is hit exactly
(s == e) by at least one pair, the 1.0 bin holds at least the 42 ordered pairs of the seven copies, at least three bins above bin 0
are non-empty, and the all-zero row's histogram is N in bin 0.

Every parity case runs on both routes (GSIM_HIST_STREAM_MAX_ROWS 0 and huge: the knobs are read per handle, so two tables).

Scores above 1: the issue that asked for this feature expected Tversky with alpha + beta < 1 to score above 1 and asked for a
non-empty bin above an edge > 1.  It cannot happen: the denominator alpha (a - c) + beta (b - c) + c is never below c for
non-negative weights, in f32 as in the reals (every term is >= 0 and rounding is monotone), so no score exceeds 1.0 --
test_asymmetric_tversky asserts that on the oracle's scores, keeps the edge above 1, and requires the bin above it to be empty on
both sides while the bin below it (the 1.0 pairs) is not."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
NT = 16
STREAM_ROWS, PAIRS = "GSIM_HIST_STREAM_MAX_ROWS", "GSIM_HIST_LAUNCH_PAIRS"
TILES, STREAM = 0, 1 << 30  # values of GSIM_HIST_STREAM_MAX_ROWS that force a route
DEFAULT_STREAM_MAX_ROWS = 32  # the knob's default
TAN = dict()
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
F = np.float32


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


def table(db, route=None, pairs=None, base=0):
    with knobs(**{STREAM_ROWS: route, PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def planted(seed, kind, n, W):
    db = O.synth_rows(seed, kind, 0, n, W)
    db[n // 3:n // 3 + 6] = db[5]  # seven identical rows: 42 ordered pairs at 1.0 besides the diagonal
    db[n // 2] = 0                 # an all-zero row: NaN against everything, itself included
    return db


_scores = {}


def score_matrix(left, db, kw=TAN, key=None):
    """S[i, j] = the oracle's score of left row i against table row j (computed once per `key`, never modified)"""
    if key is not None and (key, tuple(sorted(kw.items()))) in _scores:
        return _scores[(key, tuple(sorted(kw.items())))]
    n = len(db)

    def one(i):
        hits, _ = O.search(left[i], db, n, 0.0, kw.get("metric", O.METRIC_TANIMOTO), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        assert len(hits) == n
        row = np.empty(n, F)
        row[hits["row"]] = hits["score"]
        return row
    with ThreadPoolExecutor(NT) as pool:
        S = np.stack(list(pool.map(one, range(len(left)))))
    S.setflags(write=False)
    if key is not None:
        _scores[(key, tuple(sorted(kw.items())))] = S
    return S


def expected(S, edges, self0=None):
    """-> (hist, total) of the rule; self0: left row i is table row self0 + i and that pair is not counted"""
    e = np.asarray(edges, F)
    bins = np.searchsorted(e, S, side="right")
    hist = np.stack([np.bincount(b, minlength=len(e) + 1) for b in bins]).astype(np.uint64)
    if self0 is not None:
        for i in range(len(S)):
            hist[i, bins[i, self0 + i]] -= 1
    return hist, hist.sum(axis=0, dtype=np.uint64)


def data_edges(S, extra=(1.0,)):
    """five distinct non-zero scores that occur (quantiles of the distinct values below 1), then `extra`"""
    u = np.unique(S[(S > 0) & (S < 1)])
    assert len(u) >= 5
    picks = [u[int(q * (len(u) - 1))] for q in (0.1, 0.3, 0.5, 0.7, 0.9)]
    e = np.array(picks + list(extra), F)
    assert (np.diff(e) > 0).all()
    return e


def same(got, want, what):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
    assert np.array_equal(got[0], want[0]), (what, "hist")
    assert np.array_equal(got[1], want[1]), (what, "total")


def as_bytes(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got)


WIDTHS = [128, 160, 256, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    """n = 1200 (700 dense): four full owner tiles and one of 176 rows, whose last wave has 48; five column tiles, the last of 176."""
    W = bits // 32
    n = 1200 if kind != O.KIND_DENSE else 700
    db = planted(0xBE11 + bits + 7 * kind, kind, n, W)
    other = O.synth_rows(0x07E2 + bits + 7 * kind, kind, 0, 300, W)
    tabs = {"tiles": table(db, TILES), "stream": table(db, STREAM)}
    left = {"tiles": table(other, TILES), "stream": table(other, STREAM)}
    for kw in (TAN, TV):
        S = score_matrix(db, db, kw)
        edges = data_edges(S)
        want = expected(S, edges)
        hist = want[0]
        print(bits, kind, kw, "edges", edges.tolist(), "total", want[1].tolist())
        assert all((S == e).any() for e in edges), "every edge is hit exactly"
        assert int(hist[:, 6].sum()) >= 42 + (n - 1), "the copies' pairs (and every non-zero row's own) are in the 1.0 bin"
        assert int((want[1][1:] > 0).sum()) >= 3
        assert hist[n // 2].tolist() == [n, 0, 0, 0, 0, 0, 0], "the all-zero row"
        assert (hist.sum(axis=1) == n).all()
        want_x = expected(S, edges, self0=0)
        assert (want_x[0].sum(axis=1) == n - 1).all() and int(want_x[0][:, 6].sum()) == int(hist[:, 6].sum()) - (n - 1)
        want_o = expected(score_matrix(other, db, kw), edges)
        for route, t in tabs.items():
            what = (bits, kind, kw, route)
            st = {}
            same(t.histogram(t, edges, stats=st, **kw), want, what)
            assert st["pairs"] == n * n and st["left_rows"] == n and st["rows_streamed" if route == "stream" else "rows_tiled"] == n, st
            same(t.histogram(t, edges, exclude_self=True, **kw), want_x, what + ("exclude self",))
            same(t.histogram(left[route], edges, **kw), want_o, what + ("another table",))
            same(t.histogram(other, edges, **kw), want_o, what + ("queries",))
    for t in list(tabs.values()) + list(left.values()):
        t.close()


@pytest.mark.parametrize("bits", [1024, 256])
def test_asymmetric_tversky(bits):
    """The left row is the query: a = popc(left row) takes alpha, b = popc(table row) takes beta.  An edge above 1 is legal and its
    bin stays empty (module docstring: no score exceeds 1)."""
    n = 1200
    db = planted(0xA5E + bits, O.KIND_MORGAN, n, bits // 32)
    tabs = [table(db, TILES), table(db, STREAM)]
    for alpha, beta in ((1.0, 0.0), (0.3, 0.1)):
        kw = dict(metric=capi.METRIC_TVERSKY, alpha=alpha, beta=beta)
        S = score_matrix(db, db, kw)
        assert float(np.nanmax(S)) == 1.0
        edges = data_edges(S, extra=(1.0, 1.5))
        want = expected(S, edges)
        flipped = expected(score_matrix(db, db, dict(kw, alpha=beta, beta=alpha)), edges)
        assert not np.array_equal(want[0], flipped[0]), "the weights' roles matter on this table"
        assert int(want[1][6]) >= 42 + (n - 1) and int(want[1][7]) == 0 and int((want[1][1:] > 0).sum()) >= 3
        for t in tabs:
            same(t.histogram(t, edges, **kw), want, (bits, alpha, beta))
            same(t.histogram(t, edges, exclude_self=True, **kw), expected(S, edges, self0=0), (bits, alpha, beta, "exclude self"))
    for t in tabs:
        t.close()


MORGAN = (0xC07, O.KIND_MORGAN, 1200, 32)


def morgan():
    db = planted(*MORGAN)
    return db, score_matrix(db, db, TAN, key=MORGAN)


@pytest.mark.parametrize("route", [TILES, STREAM])
def test_128_edges(route):
    """The uniform grid k / 129 as f32: 65 LDS words of 16-bit counters per owner in the tile kernel, every cell of the coarse table
    with at most one edge."""
    db, S = morgan()
    edges = (np.arange(1, 129, dtype=F) / F(129)).astype(F)
    assert len(edges) == capi.HIST_MAX_EDGES
    want = expected(S, edges)
    assert int((want[1] > 0).sum()) >= 40
    t = table(db, route)
    for kw, w in ((TAN, want), (TV, expected(score_matrix(db, db, TV, key=MORGAN), edges))):
        same(t.histogram(t, edges, **kw), w, (route, kw))
    t.close()


@pytest.mark.parametrize("route", [TILES, STREAM])
def test_one_edge(route):
    db, S = morgan()
    t = table(db, route)
    for e in (0.3, 1.0, float(np.nextafter(F(0), F(1))), 2.0):
        want = expected(S, [e])
        same(t.histogram(t, [e]), want, (route, e))
    assert int(expected(S, [2.0])[1][1]) == 0 and int(expected(S, [1.0])[1][1]) >= 42 + 1199
    t.close()


def test_the_result_does_not_depend_on_the_route():
    db, S = morgan()
    edges = data_edges(S)
    outs = []
    for route in (TILES, STREAM):
        t = table(db, route)
        st = {}
        outs.append(as_bytes(t.histogram(t, edges, stats=st)) + as_bytes(t.histogram(t, edges, exclude_self=True, **TV)))
        assert (st["rows_tiled"], st["rows_streamed"]) == ((1200, 0) if route == TILES else (0, 1200)), st
        assert (st["tile_launches"] >= 1) == (route == TILES) and (st["stream_launches"] >= 1) == (route == STREAM), st
        t.close()
    assert outs[0] == outs[1]


def test_the_result_does_not_depend_on_the_launch_cut():
    """GSIM_HIST_LAUNCH_PAIRS = 65 536: one 256 x 256 tile to a launch of the tile kernel -- 5 owner cuts x 5 column cuts on 1200 x
    1200 -- and 256 table rows to a launch of a streaming pass: 5 launches per left row."""
    db, S = morgan()
    edges = data_edges(S)
    want = expected(S, edges)
    whole = table(db, TILES)
    st0 = {}
    a = whole.histogram(whole, edges, stats=st0)
    same(a, want, "default plan")
    whole.close()
    cut = table(db, TILES, pairs=65536)
    st = {}
    b = cut.histogram(cut, edges, stats=st)
    assert st["tile_launches"] == 25 > st0["tile_launches"] and st["pairs"] == st0["pairs"] == 1200 * 1200, (st, st0)
    assert as_bytes(a) == as_bytes(b)
    same(cut.histogram(cut, edges, exclude_self=True, row_begin=300, row_end=900), [x for x in expected(S[300:900], edges, self0=300)], "cut, a range")
    cut.close()
    cut = table(db, STREAM, pairs=256)
    st = {}
    c = cut.histogram(cut, edges, row_end=8, stats=st)
    assert st["stream_launches"] == 8 * 5 and st["rows_streamed"] == 8, st
    same(c, expected(S[:8], edges), "streaming, cut")
    same(cut.histogram(cut, edges, exclude_self=True, row_begin=700, row_end=708), expected(S[700:708], edges, self0=700), "streaming, cut, a range")
    cut.close()


@pytest.mark.parametrize("route", [TILES, STREAM])
def test_a_long_concentrated_table(route):
    """70 000 x 128-bit rows, 66 000 of them copies of one row; 300 left rows, that row among them: one owner has 66 000 pairs in a
    single bin -- more than a 16-bit counter holds, and the table is longer than 65 536 rows."""
    n, W = 70_000, 4
    db = O.synth_rows(0x10C, O.KIND_MORGAN, 0, n, W)
    copies = np.arange(n) % 35 >= 2  # 66 000 rows
    assert int(copies.sum()) == 66_000
    db[copies] = db[2]
    left = np.ascontiguousarray(db[:300])
    S = score_matrix(left, db, TAN, key="long")
    edges = np.array([0.25, 0.5, 0.75, 1.0], F)
    want = expected(S, edges)
    assert int(want[0][2, 4]) >= 66_000 and int(want[0][:, 4].max()) >= 66_000
    t = table(db, route)
    st = {}
    same(t.histogram(left, edges, stats=st), want, route)
    assert st["pairs"] == 300 * n
    same(t.histogram(t, edges, row_end=300, exclude_self=True), expected(S, edges, self0=0), (route, "exclude self"))
    t.close()


def test_against_the_rest_of_the_library():
    """No oracle: the suffix sums of a histogram row are gsim_db_search's approx at that cutoff and the lengths of the lists of
    Table.join; with exclude_self, of Table.neighbors."""
    db, S = morgan()
    edges = data_edges(S)[[1, 3, 5]]
    t = table(db)
    for kw in (TAN, TV):
        hist, _ = t.histogram(t, edges, **kw)
        hist_x, _ = t.histogram(t, edges, exclude_self=True, **kw)
        for b, e in enumerate(edges):
            suffix = hist[:, b + 1:].sum(axis=1)
            _, approx = t.search(db, 1, float(e), **kw)
            assert np.array_equal(suffix, approx.astype(np.uint64)), (kw, e, "approx")
            indptr = t.join(t, float(e), **kw)[0]
            assert np.array_equal(suffix, np.diff(indptr)), (kw, e, "join")
            assert int(suffix.sum()) > 1200, "more than the diagonal"
            nb_indptr = t.neighbors(float(e), **kw)[0]
            assert np.array_equal(hist_x[:, b + 1:].sum(axis=1), np.diff(nb_indptr)), (kw, e, "neighbors")
    t.close()


@pytest.mark.parametrize("route", [TILES, STREAM])
def test_ranges_totals_and_outputs(route):
    db, S = morgan()
    edges = data_edges(S)
    t = table(db, route)
    full = t.histogram(t, edges)
    same(full, expected(S, edges), "full")
    assert np.array_equal(full[1], full[0].sum(axis=0, dtype=np.uint64)), "total = the column sums"
    parts, totals = [], np.zeros(7, np.uint64)
    for lo, hi in ((0, 300), (300, 301), (301, 1200)):
        st = {}
        h, tot = t.histogram(t, edges, row_begin=lo, row_end=hi, stats=st)
        assert h.shape == (hi - lo, 7) and st["left_rows"] == hi - lo and st["pairs"] == (hi - lo) * 1200
        parts.append(h)
        totals += tot
    assert np.array_equal(np.concatenate(parts), full[0]) and np.array_equal(totals, full[1])
    q = np.ascontiguousarray(db[100:400])
    assert as_bytes(t.histogram(q, edges)) == as_bytes(t.histogram(t, edges, row_begin=100, row_end=400))
    assert as_bytes(t.histogram(db, edges, row_begin=100, row_end=400)) == as_bytes(t.histogram(q, edges))
    empty = t.histogram(t, edges, row_begin=17, row_end=17)
    assert empty[0].shape == (0, 7) and empty[1].tolist() == [0] * 7
    none, tot = t.histogram(t, edges, per_row=False)
    assert none is None and np.array_equal(tot, full[1])
    h, none = t.histogram(t, edges, total=False)
    assert none is None and np.array_equal(h, full[0])
    again = t.histogram(t, edges)
    assert as_bytes(again) == as_bytes(full), "a second call"
    t.close()


def test_a_row_base_changes_nothing():
    db, S = morgan()
    edges = data_edges(S)
    other = np.ascontiguousarray(db[::4])
    t, left = table(db), table(other)

    def calls():
        return [as_bytes(t.histogram(t, edges)), as_bytes(t.histogram(left, edges)),
                as_bytes(t.histogram(t, edges, exclude_self=True, row_begin=5, row_end=500)), as_bytes(t.histogram(t, edges, row_end=2))]

    plain = calls()
    t.set_row_base(1000)
    assert calls() == plain, "the table's row base"
    left.set_row_base(77)
    assert calls() == plain, "both handles' row bases"
    t.set_row_base(0)
    assert calls() == plain, "the left handle's row base"
    t.close()
    left.close()


def test_the_search_state_is_left_as_it_was():
    n, W = 3000, 32
    db = O.synth_rows(0xC0B, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    t.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 1500, 2999]])
    edges = [0.2, 0.4, 0.6]

    def searches():
        hits, approx = t.search(q, 50, 0.4)
        bufs = (np.zeros((len(q), 50), capi.HIT_DTYPE), np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint64))
        t.search_each_into(q, 50, bufs, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes() + b"".join(bufs[0][i, :bufs[1][i]].tobytes() for i in range(len(q))) + bufs[2].tobytes()

    before = searches()
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0 = t.timing()
    got = t.histogram(t, edges)
    few = t.histogram(q[:2], edges)  # (two left rows: the streaming route)
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    with pytest.raises(capi.GsimError) as e:
        t.histogram(t, [0.5, 0.5])  # a failed call ...
    assert e.value.code == -1
    assert as_bytes(t.histogram(t, edges)) == as_bytes(got)  # ... and a correct one right after it
    assert searches() == before
    _, approx = t.search(q, 1, 0.4)
    assert got[0][[7, 1500, 2999], 2:].sum(axis=1).tolist() == approx.tolist() and few[0][:, 2:].sum(axis=1).tolist() == approx[:2].tolist()
    t.close()


def test_generated_and_attached_tables():
    import torch
    n, W, seed = 2500, 5, 0xC0C
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    left = np.ascontiguousarray(db[:600])
    S = score_matrix(left, db)
    edges = data_edges(S)
    want = expected(S, edges)
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    same(g.histogram(g, edges, row_end=600), want, "generated")
    same(g.histogram(left[:2], edges), expected(S[:2], edges), "generated, streaming")
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), n, 0)
    same(a.histogram(a, edges, row_end=600), want, "attached (160 bits: zero-padded copies)")
    same(a.histogram(a, edges, row_begin=100, row_end=600, exclude_self=True), expected(S[100:], edges, self0=100), "attached, a range, exclude self")
    same(a.histogram(g, edges, row_end=600), want, "attached against generated")
    same(g.histogram(a, edges, row_begin=598, row_end=600), expected(S[598:], edges), "generated against attached, streaming")
    a.close()
    g.close()
    del ten


def test_stats():
    db, S = morgan()
    edges = data_edges(S)
    n = 1200
    t = table(db)
    for kw, nl, pairs in ((dict(), n, n * n), (dict(exclude_self=True), n, n * n - n), (dict(row_end=2), 2, 2 * n),
                          (dict(row_end=2, exclude_self=True), 2, 2 * n - 2), (dict(per_row=False), n, n * n)):
        st = {}
        h, tot = t.histogram(t, edges, stats=st, **kw)
        assert st["left_rows"] == nl and st["pairs"] == pairs == int(tot.sum()), (kw, st)
        assert st["rows_streamed"] + st["rows_tiled"] == nl and st["stream_launches"] + st["tile_launches"] >= 1, (kw, st)
        assert (st["rows_streamed"] == nl) == (nl <= DEFAULT_STREAM_MAX_ROWS), "the default route: at most GSIM_HIST_STREAM_MAX_ROWS left rows stream"
        assert st["wall_ms"] > 0 and st["stream_ms"] + st["tile_ms"] > 0 and (st["clock_mhz"] > 100) == (st["rows_tiled"] > 0), (kw, st)
    t.close()
