"""gsim_db_join / gsim_db_join_queries on the GPU: every list against the oracle (indices exactly, scores bit for bit), both
routes (streaming, tiles) forced in turn and both orders, against gsim_db_search on a 1 M-row table, against
gsim_db_neighbors for a handle joined with itself, and the overflow / multi-launch / attached-rows / search-state edges.
Everything is exact: no tolerances."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from gpusimilarity_amd.fingerprintdb import FingerprintDB

pytestmark = pytest.mark.gpu
NT = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, TILE = "2147483647", "0"  # GSIM_JOIN_STREAM_MAX_ROWS that forces either route
ROUTES = [STREAM, TILE]
ORDERS = [capi.JOIN_BY_ROW, capi.JOIN_BY_SCORE]
TAN = dict()
DICE = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
TV37 = dict(metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7)
TV73 = dict(metric=capi.METRIC_TVERSKY, alpha=0.7, beta=0.3)
SCREEN = dict(metric=capi.METRIC_TVERSKY, alpha=1.0, beta=0.0)


@contextlib.contextmanager
def knob(value):
    """The route knob is read once per handle, by gsim_db_create: set it around the creation of a table."""
    old = os.environ.get("GSIM_JOIN_STREAM_MAX_ROWS")
    if value is None:
        os.environ.pop("GSIM_JOIN_STREAM_MAX_ROWS", None)
    else:
        os.environ["GSIM_JOIN_STREAM_MAX_ROWS"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GSIM_JOIN_STREAM_MAX_ROWS", None)
        else:
            os.environ["GSIM_JOIN_STREAM_MAX_ROWS"] = old


def table(db, route=None, device=0):
    with knob(route):
        return capi.Table(db.shape[1] * 32).add_rows(db).finalize(device, 1)


def generated(seed, kind, first, n, bits=1024, route=None):
    with knob(route):
        return capi.Table(bits).generate(seed, kind, first, n, 0)


def expected(left, db, cutoff, order, metric=0, alpha=1.0, beta=1.0, row_base=0):
    """The CSR the header promises: list i = oracle search(left[i], table, k = N, cutoff) -- already in BY_SCORE order;
    stable-sorted by row for BY_ROW."""
    n = db.shape[0]
    indptr, ind, sc = [0], [], []
    for q in left:
        hits, approx = O.search(q, db, n, cutoff, metric, alpha, beta, nthreads=NT)
        assert len(hits) == approx and (hits["score"] >= np.float32(cutoff)).all()
        if order == capi.JOIN_BY_ROW:
            hits = hits[np.argsort(hits["row"], kind="stable")]
        ind.append(hits["row"].astype(np.uint32) + np.uint32(row_base))
        sc.append(hits["score"])
        indptr.append(indptr[-1] + len(hits))
    return (np.array(indptr, np.uint64), np.concatenate(ind) if ind else np.zeros(0, np.uint32),
            np.concatenate(sc) if sc else np.zeros(0, np.float32))


def same(got, want, what=None):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), what


def random_mask(rng, n, W, p):
    return np.packbits((rng.random((n, W * 32)) < p).astype(np.uint8), axis=1, bitorder="little").view(np.uint32)


def planted_inputs(bits, kind):
    """A table with an all-zero row, and left rows of every sort: the next rows of the table's own series, copies of table
    rows (1.0), table rows under a random mask (subsets: the screen's case, and scores that tell alpha from beta), unions of
    two table rows, and an all-zero left row (an empty list)."""
    W = bits // 32
    n = 1200 if kind != O.KIND_DENSE else 700
    seed = 0x10E1 + bits + 7 * kind
    db = O.synth_rows(seed, kind, 0, n, W)
    db[n // 2] = 0
    rng = np.random.default_rng(bits * 3 + kind)
    src = rng.integers(0, n, 24)
    src[src == n // 2] = 0  # (not the all-zero row)
    left = np.concatenate([O.synth_rows(seed, kind, n, 16, W), db[src[:8]], db[src[8:16]] & random_mask(rng, 8, W, 0.5),
                           db[src[16:20]] | db[src[20:24]], np.zeros((1, W), np.uint32)])
    return db, left


WIDTHS = [128, 160, 256, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]
CASES = [(TAN, 0.3), (TAN, 0.7), (DICE, 0.5), (TV37, 0.5), (TV73, 0.5), (SCREEN, 1.0)]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    db, left = planted_inputs(bits, kind)
    nl, zero = len(left), len(left) - 1
    tables = {r: table(db, r) for r in ROUTES}
    want37 = want73 = None
    for kw, cutoff in CASES:
        for order in ORDERS:
            want = expected(left, db, cutoff, order, **kw)
            assert len(want[1]) > 0, "a vacuous case"
            assert want[0][zero + 1] == want[0][zero], "the all-zero left row has an empty list"
            assert not (want[1] == db.shape[0] // 2).any(), "the all-zero table row is in nobody's list"
            for r, t in tables.items():
                st = {}
                got = t.join(left, cutoff, order=order, stats=st, **kw)
                same(got, want, (bits, kind, kw, cutoff, order, r))
                assert st["rows_streamed"] == (nl if r == STREAM else 0) and st["rows_tiled"] == (nl if r == TILE else 0)
                assert st["pairs"] == len(want[1])
            if kw is TV37 and order == capi.JOIN_BY_ROW:
                want37 = want
            if kw is TV73 and order == capi.JOIN_BY_ROW:
                want73 = want
    # the copies' lists hold their source row with 1.0
    w = expected(left[16:24], db, 1.0, capi.JOIN_BY_ROW)
    assert (np.diff(w[0].astype(np.int64)) >= 1).all() and (w[2] == 1.0).all()
    # asymmetric Tversky is asymmetric on these inputs
    assert not (np.array_equal(want37[1], want73[1]) and np.array_equal(want37[2].view(np.uint32), want73[2].view(np.uint32)))
    for t in tables.values():
        t.close()


def test_cutoff_equal_to_scores_that_occur():
    """cutoff 0.5 with c / (a + b - c) = 1/2 pairs present: they are listed (>=), and RN(1/3) ones at cutoff RN(1/3)."""
    n, W = 900, 32
    db = O.synth_rows(0x7133, O.KIND_SPARSE, 0, n, W)

    def bits(*ranges):
        x = np.zeros(W * 32, np.uint8)
        for lo, hi in ranges:
            x[lo:hi] = 1
        return np.packbits(x, bitorder="little").view(np.uint32)

    db[10] = bits((0, 40))             # 40 bits
    db[11] = bits((0, 20))             # vs 10: c = 20, a + b - c = 40: exactly 1/2
    db[12] = bits((0, 10), (40, 50))   # vs 11: c = 10, a + b - c = 30: RN(1/3)
    left = np.stack([db[10], db[11], db[12], bits((0, 20)), bits((20, 40), (100, 120))])
    for r in ROUTES:
        t = table(db, r)
        for cutoff in (np.float32(0.5), np.float32(1.0) / np.float32(3.0)):
            for order in ORDERS:
                want = expected(left, db, float(cutoff), order)
                assert (want[2] == cutoff).any(), cutoff
                same(t.join(left, float(cutoff), order=order), want, (r, cutoff, order))
        t.close()


def morgan_20k():
    n = 20000
    return O.synth_rows(0x20000, O.KIND_MORGAN, 0, n, 32), O.synth_rows(0x20000, O.KIND_MORGAN, n, 300, 32)


def test_inputs_that_are_not_vacuous():
    """Left rows that continue the table's own series (rows N ... N + 299 of the same seed) have neighbours in it -- the
    oracle's counts on this generator are asserted, so that a change of generator cannot hollow the test out."""
    db, left = morgan_20k()
    n = db.shape[0]
    tables = {r: table(db, r) for r in ROUTES}
    for cutoff, total, nonempty, longest in ((0.3, 41755, 208, 297), (0.5, 33889, 148, 279), (0.7, 3266, 81, 119), (1.0, 19, 19, 1)):
        for order in ORDERS:
            want = expected(left, db, cutoff, order)
            counts = np.diff(want[0].astype(np.int64))
            assert (int(counts.sum()), int((counts > 0).sum()), int(counts.max())) == (total, nonempty, longest)
            for r, t in tables.items():
                same(t.join(left, cutoff, order=order), want, (cutoff, order, r))
    w37 = expected(left, db, 0.6, capi.JOIN_BY_SCORE, **TV37)
    w73 = expected(left, db, 0.6, capi.JOIN_BY_SCORE, **TV73)
    assert (len(w37[1]), len(w73[1])) == (39763, 39760)
    for r, t in tables.items():
        same(t.join(left, 0.6, order=capi.JOIN_BY_SCORE, **TV37), w37, r)
        same(t.join(left, 0.6, order=capi.JOIN_BY_SCORE, **TV73), w73, r)
    differ = 0
    for i in range(50):
        a = O.search(left[i], db, n, 0.5, nthreads=NT, **TV37)[0]
        b = O.search(left[i], db, n, 0.5, nthreads=NT, **TV73)[0]
        differ += a.tobytes() != b.tobytes()
    assert differ == 33  # (by rows and scores; 19 of them by their rows alone)
    # the fingerprint screen: left row = a table row AND a random mask; its list holds every row that includes its bits
    rng = np.random.default_rng(7)
    src = rng.integers(0, n, 300)
    sub = db[src] & random_mask(rng, 300, 32, 0.35)
    assert sub.any(axis=1).all()
    want = expected(sub, db, 1.0, capi.JOIN_BY_ROW, **SCREEN)
    counts = np.diff(want[0].astype(np.int64))
    assert (counts >= 1).all() and counts.max() > 50
    for i in range(300):
        assert src[i] in want[1][int(want[0][i]):int(want[0][i + 1])]
    mirrored = expected(sub, db, 1.0, capi.JOIN_BY_ROW, metric=capi.METRIC_TVERSKY, alpha=0.0, beta=1.0)
    assert len(mirrored[1]) < len(want[1])
    for r, t in tables.items():
        same(t.join(sub, 1.0, **SCREEN), want, r)
        same(t.join(sub, 1.0, metric=capi.METRIC_TVERSKY, alpha=0.0, beta=1.0), mirrored, r)
    for t in tables.values():
        t.close()


def test_against_search_on_one_million_rows():
    """No oracle: each BY_SCORE list is the row / score of gsim_db_search's hits at the same cutoff, its length that call's
    approx.  (k = 200 000 covers the longest list at cutoff 0.3: 3 909 rows for the first 16 of these left rows.)"""
    n, k = 1_000_000, 200_000
    left = np.stack([capi.synth_row(0x20000, capi.SYNTH_MORGAN, n + i, 1024) for i in range(64)])
    for r in ROUTES:
        t = generated(0x20000, capi.SYNTH_MORGAN, 0, n, route=r)
        for cutoff in (0.3, 0.7):
            hits, approx = t.search(left, k, cutoff)
            assert int(approx.max()) <= k
            st = {}
            indptr, indices, scores = t.join(left, cutoff, order=capi.JOIN_BY_SCORE, stats=st)
            assert st["rows_streamed"] == (64 if r == STREAM else 0)
            assert np.array_equal(np.diff(indptr.astype(np.int64)), approx.astype(np.int64))
            assert int(indptr[-1]) > 0
            for i in range(64):
                lo, hi = int(indptr[i]), int(indptr[i + 1])
                assert np.array_equal(indices[lo:hi], hits[i]["row"]), (r, cutoff, i)
                assert np.array_equal(scores[lo:hi].view(np.uint32), hits[i]["score"].view(np.uint32)), (r, cutoff, i)
        t.close()


@pytest.mark.parametrize("nl", [1, 3, 255, 256, 257, 1000])
def test_route_independence(nl):
    n, W = 6000, 32
    db = O.synth_rows(0x20000, O.KIND_MORGAN, 0, n, W)
    left = O.synth_rows(0x20000, O.KIND_MORGAN, n, nl, W)
    left[0] = db[17]  # never an empty result
    ts, tt = table(db, STREAM), table(db, TILE)
    for order in ORDERS:
        for kw, cutoff in ((TAN, 0.4), (TV37, 0.5)):
            s1, s2 = {}, {}
            a = ts.join(left, cutoff, order=order, stats=s1, **kw)
            b = tt.join(left, cutoff, order=order, stats=s2, **kw)
            assert len(a[1]) > 0
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
            assert (s1["rows_streamed"], s1["rows_tiled"], s1["tile_launches"]) == (nl, 0, 0) and s1["stream_launches"] == nl
            assert (s2["rows_streamed"], s2["rows_tiled"], s2["stream_launches"]) == (0, nl, 0) and s2["tile_launches"] >= 1
            assert s1["pairs"] == s2["pairs"] == len(a[1])
            assert ts.join(left, cutoff, order=order, **kw)[1].tobytes() == a[1].tobytes()  # run to run
    want = expected(left[:40], db, 0.4, capi.JOIN_BY_SCORE)
    same(tt.join(left[:40], 0.4, order=capi.JOIN_BY_SCORE), want)
    # the default knob takes one of the two routes, and gives the same bytes
    td = table(db)
    st = {}
    d = td.join(left, 0.4, stats=st)
    assert st["rows_streamed"] + st["rows_tiled"] == nl
    assert all(x.tobytes() == y.tobytes() for x, y in zip(d, ts.join(left, 0.4)))
    for t in (ts, tt, td):
        t.close()


@pytest.mark.parametrize("route", ROUTES)
def test_left_rows_from_a_handle(route):
    n, W = 5000, 32
    db = O.synth_rows(0xA11CE, O.KIND_MORGAN, 0, n, W)
    ldb = O.synth_rows(0xA11CE, O.KIND_MORGAN, n, 1500, W)
    ldb[5] = db[99]
    t, left = table(db, route), table(ldb)
    left.set_row_base(7_000_000)  # the left handle's row base plays no part
    for order in ORDERS:
        whole = t.join(left, 0.45, order=order)
        assert len(whole[1]) > 0
        for x, y in zip(whole, t.join(ldb, 0.45, order=order)):
            assert x.tobytes() == y.tobytes()
        part = t.join(left, 0.45, order=order, row_begin=300, row_end=777)  # starts and ends inside a 256-row tile
        for x, y in zip(part, t.join(ldb[300:777], 0.45, order=order)):
            assert x.tobytes() == y.tobytes()
        assert len(part[0]) == 478 and len(part[1]) > 0
    same(t.join(left, 0.45, row_begin=0, row_end=64), expected(ldb[:64], db, 0.45, capi.JOIN_BY_ROW))
    empty = t.join(left, 0.45, row_begin=17, row_end=17)
    assert list(empty[0]) == [0] and len(empty[1]) == 0 and len(empty[2]) == 0
    empty = t.join(np.zeros((0, W), np.uint32), 0.45)
    assert list(empty[0]) == [0] and len(empty[1]) == 0
    # the table handle's row base is added to every index
    t.set_row_base(1_000_000)
    based = t.join(left, 0.45)
    plain = t.join(ldb, 0.45)
    assert np.array_equal(based[1], plain[1]) and int(based[1].min()) >= 1_000_000
    same(t.join(ldb[:64], 0.45), expected(ldb[:64], db, 0.45, capi.JOIN_BY_ROW, row_base=1_000_000))
    t.close()
    left.close()


@pytest.mark.parametrize("route", ROUTES)
def test_a_handle_joined_with_itself_is_its_neighbour_lists_plus_the_diagonal(route):
    n, W = 20000, 32
    db = O.synth_rows(0x20000, O.KIND_MORGAN, 0, n, W)
    db[1234] = 0
    t = table(db, route)
    for kw in (TAN, DICE):
        nb = t.neighbors(0.5, **kw)
        indptr, indices, scores = t.join(t, 0.5, **kw)
        nonzero = db.any(axis=1)
        counts = np.diff(indptr.astype(np.int64))
        assert np.array_equal(counts, np.diff(nb[0].astype(np.int64)) + nonzero)
        rows = np.repeat(np.arange(n), counts)
        diag = indices == rows
        assert int(diag.sum()) == int(nonzero.sum()) == n - 1 and (scores[diag] == 1.0).all()
        assert np.array_equal(indices[~diag], nb[1])
        assert np.array_equal(scores[~diag].view(np.uint32), nb[2].view(np.uint32))
    t.close()


def test_overflow_on_the_tile_route():
    """2 000 copies of one row on both sides list 4 M pairs, more than the pair buffer holds on a handle's first call: the
    launches from the first one that overflowed run again, and the result is complete."""
    n = 2000
    row = O.synth_rows(11, O.KIND_DENSE, 0, 1, 32)[0]
    db = np.tile(row, (n, 1))
    t = table(db, TILE)
    st = {}
    indptr, indices, scores = t.join(db, 0.9, stats=st)
    assert st["launches_rerun"] > 0 and st["pairs"] == n * n and st["rows_tiled"] == n, st
    assert np.array_equal(indptr, np.arange(n + 1, dtype=np.uint64) * np.uint64(n))
    assert np.array_equal(indices, np.tile(np.arange(n, dtype=np.uint32), n))
    assert (scores == 1.0).all()
    st2 = {}
    again = t.join(db, 0.9, stats=st2)  # the buffer grew: no rerun now, same bytes
    assert st2["launches_rerun"] == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip((indptr, indices, scores), again))
    g = {}
    t.neighbors(0.9, stats=g)  # ... and gsim_db_neighbors shares the grown buffer
    assert g["launches_rerun"] == 0 and g["pairs"] == n * (n - 1) // 2
    t.close()


def test_overflow_on_the_streaming_route():
    """One left row at cutoff 0.1 over 3 M Morgan-shaped rows keeps well over 2 M of them: the first call on the handle
    overflows the pair buffer inside the pass.  Exact: the count is gsim_db_search's approx, a sample of rows is checked
    against the oracle, and the list is sorted and free of duplicates."""
    n, seed = 3_000_000, 0x20000
    t = generated(seed, capi.SYNTH_MORGAN, 0, n, route=STREAM)
    q = capi.synth_row(seed, capi.SYNTH_MORGAN, n + 3, 1024)
    st = {}
    indptr, indices, scores = t.join(q, 0.1, stats=st)
    assert st["launches_rerun"] > 0 and st["rows_streamed"] == 1 and st["pairs"] == len(indices) > 2_000_000, st
    _, approx = t.search(q, 10, 0.1)
    assert int(indptr[1]) == int(approx[0]) == len(indices)
    assert (np.diff(indices.astype(np.int64)) > 0).all() and int(indices[-1]) < n
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(n, 3000, replace=False))
    rows = np.stack([capi.synth_row(seed, capi.SYNTH_MORGAN, int(r), 1024) for r in sample])
    hits, _ = O.search(q, rows, len(rows), 0.1, nthreads=NT)
    hits = hits[np.argsort(hits["row"], kind="stable")]
    assert len(hits) > 0
    pos = np.searchsorted(indices, sample)
    listed = (pos < len(indices)) & (indices[np.minimum(pos, len(indices) - 1)] == sample)
    assert np.array_equal(np.flatnonzero(listed), hits["row"])
    assert np.array_equal(scores[pos[listed]].view(np.uint32), hits["score"].view(np.uint32))
    st2 = {}
    again = t.join(q, 0.1, stats=st2)
    assert st2["launches_rerun"] == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip((indptr, indices, scores), again))
    by_score = t.join(q, 0.1, order=capi.JOIN_BY_SCORE)
    o = np.lexsort((indices, -scores.astype(np.float64)))
    assert np.array_equal(by_score[1], indices[o]) and np.array_equal(by_score[2].view(np.uint32), scores[o].view(np.uint32))
    t.close()


def test_multi_launch_passes_give_the_same_result(tmp_path):
    """Test-hooks build, GSIM_TEST_JOIN_LAUNCH_ROWS = 16384: every pass over 50 000 rows runs in 4 launches."""
    from conftest import hooks_env, HOOKS_LIB
    assert os.path.exists(HOOKS_LIB)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, oracle_lib as O; from gpusimilarity_amd import capi\n"
            "out = {}\n"
            "for bits in (1024, 160, 896):\n"
            "    db = O.synth_rows(0x3A17 + bits, O.KIND_MORGAN, 0, 50000, bits // 32)\n"
            "    left = O.synth_rows(0x3A17 + bits, O.KIND_MORGAN, 50000, 5, bits // 32)\n"
            "    left[0] = db[49999]\n"
            "    t = capi.Table(bits).add_rows(db).finalize(0, 1)\n"
            "    for order in (0, 1):\n"
            "        st = {}\n"
            "        r = t.join(left, 0.3, order=order, stats=st)\n"
            "        out.update({'%%d_%%d_%%d' %% (bits, order, i): x for i, x in enumerate(r)})\n"
            "        out['%%d_%%d_launches' %% (bits, order)] = np.array(st['stream_launches'])\n"
            "    t.close()\n"
            "np.savez(sys.argv[1], **out)\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    runs = {}
    for cap in ("16384", None):
        env = hooks_env(GSIM_JOIN_STREAM_MAX_ROWS=STREAM, **({"GSIM_TEST_JOIN_LAUNCH_ROWS": cap} if cap else {}))
        path = str(tmp_path / ("run_%s.npz" % cap))
        r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        runs[cap] = np.load(path)
    capped, whole = runs["16384"], runs[None]
    for bits in (1024, 160, 896):
        for order in (0, 1):
            assert int(whole["%d_%d_launches" % (bits, order)]) == 5 and int(capped["%d_%d_launches" % (bits, order)]) == 20, bits
            assert len(whole["%d_%d_1" % (bits, order)]) > 0
            for i in range(3):
                k = "%d_%d_%d" % (bits, order, i)
                assert capped[k].tobytes() == whole[k].tobytes(), k


@pytest.mark.parametrize("bits", [1024, 160])
@pytest.mark.parametrize("route", ROUTES)
def test_attached_device_rows_on_either_side(bits, route):
    """Rows borrowed from torch tensors (gsim_db_attach_device_rows) as the table and as the left handle."""
    import torch
    n, nl, W = 2500, 700, bits // 32
    db = O.synth_rows(0xA77 + bits, O.KIND_MORGAN, 0, n, W)
    ldb = O.synth_rows(0xA77 + bits, O.KIND_MORGAN, n, nl, W)
    ldb[3] = db[77]
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    lten = torch.from_numpy(ldb.view(np.int32).copy()).to("cuda:0")
    with knob(route):
        t = capi.Table(bits)
    t.attach_device_rows(ten.data_ptr(), n, 0)
    left = capi.Table(bits)
    left.attach_device_rows(lten.data_ptr(), nl, 0)
    u = table(db, route)
    for order in ORDERS:
        got = t.join(left, 0.4, order=order)
        part = t.join(left, 0.4, order=order, row_begin=100, row_end=613)
        assert len(got[1]) > 0
        for x, y in zip(got, u.join(ldb, 0.4, order=order)):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(part, u.join(ldb[100:613], 0.4, order=order)):
            assert x.tobytes() == y.tobytes()
    same(t.join(left, 0.4, row_begin=0, row_end=50), expected(ldb[:50], db, 0.4, capi.JOIN_BY_ROW))
    t.close()
    left.close()
    u.close()
    del ten, lten


@pytest.mark.parametrize("route", ROUTES)
def test_the_search_state_survives(route):
    n, W = 3000, 16
    db = O.synth_rows(0xA11, O.KIND_MORGAN, 0, n, W)
    ldb = O.synth_rows(0xA11, O.KIND_MORGAN, n, 400, W)
    t, left = table(db, route), table(ldb)
    q = db[[7, 1500, 2999]]
    before, lbefore, nb = t.search(q, 50, 0.4), left.search(q, 50, 0.2), t.neighbors(0.55)
    a = t.join(left, 0.5)
    b = t.join(ldb, 0.5, order=capi.JOIN_BY_SCORE)
    assert len(a[1]) > 0 and len(b[1]) == len(a[1])
    after, lafter, nb2 = t.search(q, 50, 0.4), left.search(q, 50, 0.2), t.neighbors(0.55)
    for x, y in ((before, after), (lbefore, lafter)):
        for h0, h1 in zip(x[0], y[0]):
            assert h0.tobytes() == h1.tobytes()
        assert np.array_equal(x[1], y[1])
    for x, y in zip(nb, nb2):
        assert x.tobytes() == y.tobytes()
    t.close()
    left.close()


def test_error_codes_on_the_gpu():
    db = O.synth_rows(5, O.KIND_SPARSE, 0, 512, 32)
    t = table(db)
    for bad in (0.0, -1.0, 1.01):
        with pytest.raises(capi.GsimError) as e:
            t.join(db[:2], bad)
        assert e.value.code == -1
    f = capi.Table(1024).add_rows(db).set_fold_factor(2).finalize(0, 1)
    for tab, lf in ((f, db[:2]), (f, t), (t, f)):
        with pytest.raises(capi.GsimError) as e:
            tab.join(lf, 0.5)
        assert e.value.code == -5
    f.close()
    L = capi.load()
    import ctypes as C
    g = C.c_void_p()
    capi.check(L.gsim_db_neighbors(t._h, 0.5, 0, 1.0, 1.0, 0, 512, C.byref(g)))
    assert L.gsim_graph_get_join_stats(g, C.byref(capi.GsimJoinStats())) == -1  # not a join's result
    L.gsim_graph_destroy(g)
    st = {}
    t.join(db[:2], 0.5, stats=st)
    assert st["pairs"] >= 2 and st["wall_ms"] > 0
    t.close()
    # a multi-shard handle: two logical devices on one GPU (the test-hooks build of the library)
    from conftest import hooks_env, HOOKS_LIB
    assert os.path.exists(HOOKS_LIB)
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from gpusimilarity_amd import capi\n"
            "t = capi.Table(1024).add_rows(np.ones((512, 32), np.uint32)).finalize(0, 2)\n"
            "u = capi.Table(1024).add_rows(np.ones((512, 32), np.uint32)).finalize(0, 1)\n"
            "assert t.shard_count() == 2\n"
            "for a, b in ((t, np.ones((2, 32), np.uint32)), (t, u), (u, t)):\n"
            "    try:\n        a.join(b, 0.5)\n    except capi.GsimError as e:\n        print('code', e.code)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=hooks_env(GSIM_TEST_ALIAS_DEVICES="2"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("code -5") == 3, r.stdout + r.stderr


def test_fingerprintdb_join_and_screen():
    n, W = 5000, 32
    db = O.synth_rows(0x5EED, O.KIND_MORGAN, 0, n, W)
    fdb = FingerprintDB(1024, n, "k", [db], [b"s%d" % i for i in range(n)], [b"i%d" % i for i in range(n)])
    fdb.copyToGPU()
    left = O.synth_rows(0x5EED, O.KIND_MORGAN, n, 100, W)
    same(fdb.join(left, 0.5, order=capi.JOIN_BY_SCORE), expected(left, db, 0.5, capi.JOIN_BY_SCORE))
    other = FingerprintDB(1024, 100, "k", [left], [b"s%d" % i for i in range(100)], [b"i%d" % i for i in range(100)])
    other.copyToGPU()
    same(fdb.join(other, 0.5), expected(left, db, 0.5, capi.JOIN_BY_ROW))
    rng = np.random.default_rng(1)
    q = db[321] & random_mask(rng, 1, W, 0.4)[0]
    rows = fdb.screen(q)
    want = np.flatnonzero(((db & q) == q).all(axis=1)).astype(np.uint32)
    assert q.any() and 321 in rows and np.array_equal(rows, want)
