"""Nearest-centre assignment on the GPU (gsim_db_assign).

Expected values: tests/kmeans_rule.py -- the oracle's score matrix (centre as the query), numpy's arg-max down every column (the
first, i.e. lowest, centre among equal f32 scores).  Every comparison is exact: view(np.uint32) for the scores.

Data: tables of N = 3000 rows (no multiple of 32 or 128: 24 row blocks of the kernel, the last of 56 rows) synth_rows(21, kind, 0,
N, W) and m = 300 centres (three centre blocks, the last of 44): 100 table rows (a score of 1.0 exists) and 200 rows of another seed.
Planted: centre 7 is a copy of centre 3, one all-zero and one all-ones centre, an all-zero and an all-ones row, six identical rows.
Asserted on the EXPECTED result before anything is compared: at least 20 distinct labels, a row whose maximum two centres attain
with the lower one expected, no row labelled 7, the zero row at (0, 0.0)."""
import contextlib
import os

import numpy as np
import pytest

import kmeans_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32
PAIRS = "GSIM_ASSIGN_LAUNCH_PAIRS"
N, M = 3000, 300
FROM_TABLE = 30 * np.arange(100)          # centre c < 100 is table row 30 c
COPY_OF, COPY = 3, 7
ZERO_C, ONES_C = 150, 151
ZERO_R, ONES_R, SAME_R = 1501, 1502, range(2001, 2007)
TV = R.tv


@contextlib.contextmanager
def knob(value):
    old = os.environ.get(PAIRS)
    if value is None:
        os.environ.pop(PAIRS, None)
    else:
        os.environ[PAIRS] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(PAIRS, None)
        else:
            os.environ[PAIRS] = old


def table(db, pairs=None):
    with knob(pairs):  # (read once per handle, by gsim_db_create)
        return capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)


_data, _scores = {}, {}


def data(kind, W):
    """-> (table rows, centres), planted; made once per (kind, W), never modified"""
    if (kind, W) not in _data:
        db = O.synth_rows(21, kind, 0, N, W)
        db[ZERO_R] = 0
        db[ONES_R] = 0xFFFFFFFF
        db[SAME_R.start:SAME_R.stop] = db[77]
        db[30 * COPY_OF, 0] |= 1  # (never an all-zero row: its score against its own copy among the centres is 1.0)
        cen = np.concatenate([db[FROM_TABLE], O.synth_rows(22, kind, 0, M - 100, W)])
        cen[COPY] = cen[COPY_OF]
        cen[ZERO_C] = 0
        cen[ONES_C] = 0xFFFFFFFF
        db.setflags(write=False)
        cen.setflags(write=False)
        _data[(kind, W)] = (db, cen)
    return _data[(kind, W)]


def expected(kind, W, kw=R.TAN):
    key = (kind, W, tuple(sorted(kw.items())))
    if key not in _scores:
        db, cen = data(kind, W)
        _scores[key] = R.score_matrix(cen, db, kw)
    return _scores[key]


def check_expected(S, label, score):
    assert S.shape == (M, N) and label.shape == (N,) and score.dtype == F
    assert len(np.unique(label)) >= 20, "at least 20 distinct labels"
    tied = R.tied(S)
    assert len(tied) >= 1, "a row whose maximum two centres attain"
    for i in tied[:50]:
        assert label[i] == np.flatnonzero(S[:, i] == S[:, i].max())[0], "the lower one is expected"
    assert S[COPY_OF, 30 * COPY_OF] == 1.0 == S[COPY, 30 * COPY_OF] and label[30 * COPY_OF] == COPY_OF, "the copy ties at 1.0"
    assert (label != COPY).all(), "no row is labelled 7: centre 3 ties with it everywhere"
    assert label[ZERO_R] == 0 and score[ZERO_R].view(np.uint32) == 0, "the zero row is (0, 0.0)"
    assert label[ONES_R] == ONES_C and score[ONES_R] == 1.0


def same(got, want, what):
    gl, gs = got
    wl, ws = want
    assert gl.dtype == np.uint32 and gs.dtype == F and gl.shape == wl.shape and gs.shape == ws.shape, what
    bad = np.flatnonzero((gl != wl) | (gs.view(np.uint32) != ws.view(np.uint32)))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), gl[bad[:5]].tolist(), wl[bad[:5]].tolist(), gs[bad[:5]].tolist(), ws[bad[:5]].tolist())


WIDTHS = [32, 96, 160, 256, 1024, 1056, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]
K1024 = (O.KIND_MORGAN, 32)


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_rule(bits, kind):
    """One word, padded widths (32, 96, 160, 1056), one 256-bit group, whole groups, the maximum."""
    W = bits // 32
    db, cen = data(kind, W)
    S = expected(kind, W)
    want = R.assign(S)
    check_expected(S, *want)
    t = table(db)
    st = {}
    got = t.assign(cen, stats=st)
    same(got, want, (bits, kind))
    assert st["rows"] == N and st["centres"] == M and st["pairs"] == M * N and st["launches"] >= 1, st
    assert st["kernel_ms"] > 0 and st["wall_ms"] > 0 and st["clock_mhz"] > 100, st
    # a second path on the same GPU (not the expected value): the arg-max of the dense matrix
    G = t.scores(cen)
    assert np.array_equal(got[0], np.argmax(G, axis=0).astype(np.uint32)), (bits, kind, "against Table.scores")
    assert np.array_equal(got[1].view(np.uint32), G.max(axis=0).view(np.uint32))
    t.close()


def test_edge_shapes():
    """Centre counts around the 32-wide MFMA tile and the 128-wide block; ranges that start and end inside row blocks."""
    db, cen = data(*K1024)
    S = expected(*K1024)
    t = table(db)
    for m in (1, 2, 31, 32, 33, 127, 128, 129, 300):
        for a, b in ((0, 1), (5, 37), (31, 161), (2999, 3000), (0, 3000)):
            same(t.assign(cen[:m], row_begin=a, row_end=b), R.assign(S[:m, a:b]), (m, a, b))
    lab, sc = t.assign(cen, row_begin=9, row_end=9)
    assert len(lab) == 0 and len(sc) == 0
    t.close()


def test_tversky():
    db, cen = data(*K1024)
    t = table(db)
    tan = t.assign(cen)
    same(tan, R.assign(expected(*K1024)), "Tanimoto")
    seen = []
    for kw in (TV(0.5, 0.5), TV(0.3, 0.7), TV(0.0, 0.0)):
        S = expected(*K1024, kw)
        want = R.assign(S)
        assert len(R.tied(S)) >= 1 and want[0][ZERO_R] == 0 and want[1][ZERO_R] == 0.0
        same(t.assign(cen, **kw), want, kw)
        seen.append(want[0])
    assert not np.array_equal(seen[0], seen[1]), "the asymmetric weights change the assignment"
    assert set(np.unique(expected(*K1024, TV(0.0, 0.0)))) == {0.0, 1.0}, "Tversky (0, 0): c / c"
    same(t.assign(cen, **TV(1.0, 1.0)), tan, "Tversky (1, 1) is Tanimoto bit for bit")
    same(t.assign(cen, **TV(0.7, 0.3)), R.assign(expected(*K1024, TV(0.7, 0.3))), "the weights swapped")
    t.close()


@pytest.mark.parametrize("bits", [1024, 160])
def test_launch_cuts_ranges_and_repeats(bits):
    kind, W = O.KIND_MORGAN, bits // 32
    db, cen = data(kind, W)
    want = R.assign(expected(kind, W))
    t = table(db)
    st0 = {}
    whole = t.assign(cen, stats=st0)
    same(whole, want, "default plan")
    assert st0["launches"] == 1, st0
    again = t.assign(cen)
    assert again[0].tobytes() == whole[0].tobytes() and again[1].tobytes() == whole[1].tobytes(), "a second call"
    parts = [t.assign(cen, row_begin=0, row_end=1300), t.assign(cen, row_begin=1300, row_end=N)]
    same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), whole, "two ranges that partition the table")
    t.set_row_base(1000)
    same(t.assign(cen, row_begin=5, row_end=900), (whole[0][5:900], whole[1][5:900]), "the row base plays no part")
    t.close()
    for pairs, launches in ((1, (N + 127) // 128), (M * 128 * 10, 3)):  # one row block a launch; 1280 rows a launch: cuts mid-table
        cut = table(db, pairs=pairs)
        st = {}
        got = cut.assign(cen, stats=st)
        assert st["launches"] == launches and st["pairs"] == M * N, (pairs, st)
        assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes(), pairs
        cut.close()


def test_attached_and_generated_tables():
    import torch
    W, seed, n = 5, 0xA55, 3000  # 160 bits: the slab's zero-padded copy
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    cen = np.ascontiguousarray(db[::37][:70])
    want = R.assign(R.score_matrix(cen, db))
    assert len(np.unique(want[0])) >= 20
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), n, 0)
    same(g.assign(cen), want, "generated")
    same(a.assign(cen), want, "attached")
    same(a.assign(cen, row_begin=100, row_end=2900), (want[0][100:2900], want[1][100:2900]), "attached, a range")
    for x in (g, a):
        x.close()
    del ten


def test_the_search_state_is_left_as_it_was():
    db, cen = data(*K1024)
    t = table(db)
    t.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 1500, 2999]])

    def searches():
        hits, approx = t.search(q, 50, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0 = t.timing()
    got = t.assign(cen)
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    with pytest.raises(capi.GsimError) as e:
        t.assign(cen, row_end=N + 1)  # a failed call ...
    assert e.value.code == -1
    same(t.assign(cen), got, "... and a correct one right after it")
    assert searches() == before
    t.close()
