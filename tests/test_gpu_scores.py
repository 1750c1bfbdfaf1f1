"""Dense similarity matrices on the GPU (gsim_db_scores, gsim_db_scores_queries, gsim_db_scores_device).

Expected values: for left row i the oracle's scores of row i against every table row (oracle_lib.search with k = N at cutoff 0,
scattered by row as test_gpu_histogram.py builds its score matrix: every row comes back, NaN as 0.0).  Every comparison is
view(np.uint32) equality: no tolerances anywhere.

Data: a 700-row table synth_rows(11, kind, 0, 700, W) and 300 left rows synth_rows(12, kind, 0, 300, W) with rows planted on both
sides: left rows 0..2 and table rows 233..238 equal table row 5, one all-zero row and one all-ones row on each side.  Asserted on
the EXPECTED matrix before anything is compared: at least 20 distinct values, an off-diagonal 1.0, a 0.0 that comes from 0 / 0,
and the all-ones pair at 1.0.  300 x 700 is 3 x 6 blocks of the kernel's 128 x 128, the last of either side partial (44 and 60
rows)."""
import contextlib
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
NT = 16
F = np.float32
PAIRS, STAGE = "GSIM_SCORES_LAUNCH_PAIRS", "GSIM_SCORES_STAGE_BYTES"
TAN = dict()
FILL = 0x7FC12345  # a NaN's bit pattern: no score ever equals it
N, NL = 700, 300
COPIES, ZERO_T, ONES_T = range(233, 239), 350, 351  # planted table rows
ZERO_L, ONES_L = 150, 151                           # planted left rows


def tv(alpha, beta):
    return dict(metric=capi.METRIC_TVERSKY, alpha=alpha, beta=beta)


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


def table(db, pairs=None, stage=None):
    with knobs(**{PAIRS: pairs, STAGE: stage}):
        return capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)


_data = {}


def data(kind, W):
    """-> (table rows, left rows), planted; made once per (kind, W), never modified"""
    if (kind, W) not in _data:
        db = O.synth_rows(11, kind, 0, N, W)
        left = O.synth_rows(12, kind, 0, NL, W)
        db[COPIES.start:COPIES.stop] = db[5]
        left[0:3] = db[5]
        db[ZERO_T] = 0
        left[ZERO_L] = 0
        db[ONES_T] = 0xFFFFFFFF
        left[ONES_L] = 0xFFFFFFFF
        db.setflags(write=False)
        left.setflags(write=False)
        _data[(kind, W)] = (db, left)
    return _data[(kind, W)]


_scores = {}


def score_matrix(left, db, kw=TAN, key=None):
    """S[i, j] = the oracle's score of left row i against table row j (computed once per `key`, never modified)"""
    k = (key, tuple(sorted(kw.items())))
    if key is not None and k in _scores:
        return _scores[k]
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
        _scores[k] = S
    return S


def expected(kind, W, kw=TAN, self_=False):
    db, left = data(kind, W)
    return score_matrix(db if self_ else left, db, kw, key=(kind, W, self_))


def popc(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=-1).sum(axis=-1)


def check_expected(S, kind, W, zero_weights=False):
    """zero_weights: Tversky (0, 0), whose denominator is c itself -- every score is c / c = 1.0, or 0.0 for c == 0: two values"""
    db, left = data(kind, W)
    assert S.shape == (NL, N) and S.dtype == F
    if zero_weights:
        assert np.unique(S).tolist() == [0.0, 1.0] and 0.05 < float(S.mean()) < 0.999
    else:
        assert len(np.unique(S)) >= 20, "at least 20 distinct values"
    ones = np.argwhere(S == 1.0)
    assert ((ones[:, 0] != ones[:, 1]).any()), "an off-diagonal 1.0"
    assert all(S[i, j] == 1.0 for i in range(3) for j in COPIES)
    assert popc(left[ZERO_L]) == 0 and popc(db[ZERO_T]) == 0 and S[ZERO_L, ZERO_T].view(np.uint32) == 0, "0 / 0 is 0.0f"
    assert popc(left[ONES_L]) == W * 32 == popc(db[ONES_T]) and S[ONES_L, ONES_T] == 1.0, "c = a = b = fp_bits"
    assert not np.isnan(S).any() and float(S.min()) >= 0.0 and float(S.max()) <= 1.0


def same(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [(float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:5]])


WIDTHS = [32, 128, 160, 256, 1024, 1056, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    """One word, padded widths (32, 128, 160, 1056), one 256-bit group, five groups (1056: not a power of two), the maximum."""
    W = bits // 32
    db, left = data(kind, W)
    S = expected(kind, W)
    check_expected(S, kind, W)
    t, lt = table(db), table(left)
    same(t.scores(lt), S, (bits, kind, "handle"))
    same(t.scores(left), S, (bits, kind, "queries"))
    t.close()
    lt.close()


@pytest.mark.parametrize("bits", [1024, 160])
def test_metrics(bits):
    W, kind = bits // 32, O.KIND_MORGAN
    db, left = data(kind, W)
    asym = expected(kind, W, tv(0.3, 0.7), self_=True)
    assert not np.array_equal(asym, asym.T), "Tversky (0.3, 0.7) of the table against itself is not symmetric"
    t, lt = table(db), table(left)
    for kw in (tv(0.5, 0.5), tv(0.3, 0.7), tv(0.0, 0.0)):
        S = expected(kind, W, kw)
        check_expected(S, kind, W, zero_weights=kw["alpha"] == 0.0)
        same(t.scores(lt, **kw), S, (bits, kw))
    same(t.scores(t, **tv(0.3, 0.7)), asym, (bits, "asymmetric, the table against itself"))
    same(t.scores(lt, **tv(0.7, 0.3)), expected(kind, W, tv(0.7, 0.3)), (bits, "the weights swapped"))
    assert not np.array_equal(expected(kind, W, tv(0.7, 0.3)), expected(kind, W, tv(0.3, 0.7)))
    tan = t.scores(lt)
    same(tan, expected(kind, W), (bits, "Tanimoto"))
    same(t.scores(lt, **tv(1.0, 1.0)), tan, (bits, "Tversky (1, 1) is Tanimoto bit for bit"))
    t.close()
    lt.close()


K1024 = (O.KIND_MORGAN, 32)


def test_edge_shapes():
    """Slices of one oracle matrix: block edges of the 128 x 128 workgroup block and of its 32 x 32 MFMA tiles."""
    db, left = data(*K1024)
    S = expected(*K1024)
    t, lt = table(db), table(left)
    for nl in (1, 31, 33, 65, 129, 257):
        for nr in (1, 31, 33, 65, 129, 257, 700):
            same(t.scores(lt, row_end=nl, col_end=nr), S[:nl, :nr], (nl, nr))
    for nl, nr in ((1, 1), (33, 129), (129, 33), (293, 687)):
        same(t.scores(lt, row_begin=7, row_end=7 + nl, col_begin=13, col_end=13 + nr), S[7:7 + nl, 13:13 + nr], ("from (7, 13)", nl, nr))
        same(t.scores(left, row_begin=7, row_end=7 + nl, col_begin=13, col_end=13 + nr), S[7:7 + nl, 13:13 + nr], ("queries from (7, 13)", nl, nr))
    one = table(np.ascontiguousarray(db[13:14]))
    same(one.scores(lt), S[:, 13:14], "a one-row table")
    assert one.scores(lt).shape == (NL, 1)
    short = table(np.ascontiguousarray(db[:200]))
    same(short.scores(lt), S[:, :200], "a left side longer than the table")
    for empty in (t.scores(lt, row_begin=9, row_end=9), t.scores(lt, col_begin=9, col_end=9), t.scores(left[:0])):
        assert empty.size == 0 and empty.dtype == F
    assert t.scores(lt, row_begin=9, row_end=9).shape == (0, N) and t.scores(lt, col_begin=9, col_end=9).shape == (NL, 0)
    for x in (t, lt, one, short):
        x.close()


def test_ld_larger_than_nr_leaves_the_padding_alone():
    import torch
    db, left = data(*K1024)
    S = expected(*K1024)
    t, lt = table(db), table(left)
    L = capi.load()
    fp = C.POINTER(C.c_float)
    for (l0, l1, r0, r1, ld) in ((0, NL, 0, N, N + 1), (7, 140, 13, 142, 200), (0, 3, 0, 1, 64)):
        nl, nr = l1 - l0, r1 - r0
        buf = np.full((nl, ld), FILL, np.uint32)
        assert L.gsim_db_scores(t._h, lt._h, l0, l1, r0, r1, 0, 1.0, 1.0, buf.ctypes.data_as(fp), ld, None) == 0
        same(buf[:, :nr].view(F), S[l0:l1, r0:r1], ("host", ld))
        assert (buf[:, nr:] == FILL).all(), ("host padding", ld)
        q = np.ascontiguousarray(left[l0:l1])
        buf = np.full((nl, ld), FILL, np.uint32)
        assert L.gsim_db_scores_queries(t._h, q.ctypes.data_as(C.POINTER(C.c_uint32)), nl, r0, r1, 0, 1.0, 1.0, buf.ctypes.data_as(fp), ld, None) == 0
        same(buf[:, :nr].view(F), S[l0:l1, r0:r1], ("host, queries", ld))
        assert (buf[:, nr:] == FILL).all(), ("host padding, queries", ld)
        ten = torch.full((nl, ld), FILL, dtype=torch.int32, device="cuda:0")
        assert t.scores(lt, row_begin=l0, row_end=l1, col_begin=r0, col_end=r1, out_ptr=ten.data_ptr(), ld=ld) is None
        got = ten.cpu().numpy().view(np.uint32)
        same(got[:, :nr].view(F), S[l0:l1, r0:r1], ("device", ld))
        assert (got[:, nr:] == FILL).all(), ("device padding", ld)
    t.close()
    lt.close()


def test_blocks_concatenate():
    db, left = data(*K1024)
    S = expected(*K1024)
    t, lt = table(db), table(left)
    rows, cols = (0, 100, 129, NL), (0, 128, 300, N)  # a 3 x 3 grid of unequal blocks
    grid = [[t.scores(lt, row_begin=rows[i], row_end=rows[i + 1], col_begin=cols[j], col_end=cols[j + 1]) for j in range(3)] for i in range(3)]
    whole = t.scores(lt)
    same(np.block(grid), whole, "3 x 3 blocks")
    same(whole, S, "the whole")
    assert whole.tobytes() == t.scores(lt).tobytes(), "a second call"
    t.close()
    lt.close()


def test_device_output_on_a_torch_stream():
    import torch
    db, left = data(*K1024)
    S = expected(*K1024)
    t, lt = table(db), table(left)
    host = t.scores(lt)
    st = torch.cuda.Stream(device=0)
    assert st.cuda_stream != 0
    t.set_stream(st.cuda_stream)
    out = torch.zeros((NL, N), dtype=torch.float32, device="cuda:0")
    stats = {}
    with torch.cuda.stream(st):
        assert t.scores(lt, out_ptr=out.data_ptr(), stats=stats) is None
    # the call returned with its stream idle: the tensor is usable on any stream straight away
    hi, lo = float(out.max().item()), float(out.min().item())
    got = out.cpu().numpy()
    assert got.tobytes() == host.tobytes(), "device output == host output"
    same(got, S, "device output")
    assert (hi, lo) == (float(S.max()), float(S.min())) == (1.0, 0.0)
    assert stats["slabs"] == 0 and stats["launches"] >= 1 and stats["d2h_ms"] == 0.0, stats
    t.close()
    lt.close()


def test_left_is_the_table():
    for bits in (1024, 160):
        W = bits // 32
        db, _ = data(O.KIND_MORGAN, W)
        S = expected(O.KIND_MORGAN, W, self_=True)
        t = table(db)
        got = t.scores(t)
        same(got, S, (bits, "self"))
        diag = np.diag(got)
        want = np.ones(N, F)
        want[ZERO_T] = 0.0
        assert diag.view(np.uint32).tolist() == want.view(np.uint32).tolist(), "the diagonal: 1.0, 0.0 for the all-zero row"
        assert got.tobytes() == np.ascontiguousarray(got.T).tobytes(), "Tanimoto's matrix equals its transpose bitwise"
        same(t.scores(t, row_begin=100, row_end=400, col_begin=50, col_end=650), S[100:400, 50:650], (bits, "self, ranges"))
        t.close()


def test_the_result_does_not_depend_on_launches_or_slabs():
    db, left = data(*K1024)
    S = expected(*K1024)
    t, lt = table(db), table(left)
    st0 = {}
    whole = t.scores(lt, stats=st0)
    same(whole, S, "default plan")
    assert st0["launches"] == 1 and st0["slabs"] == 1, st0
    t.close()
    cut = table(db, pairs=1)  # one 128 x 128 block to a launch: 3 x 6
    st = {}
    got = cut.scores(lt, stats=st)
    assert st["launches"] == 18 > st0["launches"] and st["slabs"] == 1 and st["pairs"] == NL * N, st
    assert got.tobytes() == whole.tobytes()
    assert cut.scores(left).tobytes() == whole.tobytes()
    cut.close()
    slabs = table(db, stage=100 * N * 4)  # 100 left rows to a slab
    st = {}
    got = slabs.scores(lt, stats=st)
    assert st["slabs"] == 3 and st["launches"] == 3, st
    assert got.tobytes() == whole.tobytes()
    buf = np.full((NL, N + 3), FILL, np.uint32)
    assert capi.load().gsim_db_scores(slabs._h, lt._h, 0, NL, 0, N, 0, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_float)), N + 3, None) == 0
    assert buf[:, :N].tobytes() == whole.tobytes() and (buf[:, N:] == FILL).all(), "slabs with ld > nr"
    slabs.close()
    both = table(db, pairs=1, stage=1)  # a row to a slab, a block to a launch
    st = {}
    got = both.scores(lt, row_end=5, stats=st)
    assert st["slabs"] == 5 and st["launches"] == 5 * 6, st
    assert got.tobytes() == whole[:5].tobytes()
    both.close()
    lt.close()


def test_entry_points_and_table_sources():
    import torch
    W, seed = 5, 0xC0C  # 160 bits: zero-padded copies of both sides
    n, nl = 900, 260
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    left = np.ascontiguousarray(db[300:300 + nl])
    S = score_matrix(left, db)
    assert len(np.unique(S)) >= 20
    t = table(db)
    same(t.scores(left), S, "queries")
    same(t.scores(t, row_begin=300, row_end=300 + nl), S, "handle")
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), n, 0)
    same(g.scores(g, row_begin=300, row_end=300 + nl), S, "generated")
    same(a.scores(a, row_begin=300, row_end=300 + nl), S, "attached")
    same(a.scores(g, row_begin=300, row_end=300 + nl), S, "attached against generated")
    same(g.scores(a, row_begin=300, row_end=300 + nl, col_begin=100, col_end=777), S[:, 100:777], "generated against attached, a range")
    same(t.scores(a, row_begin=300, row_end=300 + nl), S, "host-made against attached")
    out = torch.zeros((nl, n), dtype=torch.float32, device="cuda:0")
    g.scores(a, row_begin=300, row_end=300 + nl, out_ptr=out.data_ptr())
    same(out.cpu().numpy(), S, "device output, generated against attached")

    def calls():
        return [t.scores(g, row_begin=300, row_end=300 + nl).tobytes(), g.scores(t, row_begin=5, row_end=40, col_begin=3, col_end=500).tobytes(),
                t.scores(left).tobytes()]

    plain = calls()
    t.set_row_base(1000)
    assert calls() == plain, "the table's row base"
    g.set_row_base(77)
    assert calls() == plain, "both handles' row bases"
    t.set_row_base(0)
    assert calls() == plain, "the left handle's row base"
    for x in (t, g, a):
        x.close()
    del ten


def test_the_search_state_is_left_as_it_was():
    n, W = 3000, 32
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
    got = t.scores(t, row_end=500)
    few = t.scores(q)
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    with pytest.raises(capi.GsimError) as e:
        t.scores(t, col_end=n + 1)  # a failed call ...
    assert e.value.code == -1
    assert t.scores(t, row_end=500).tobytes() == got.tobytes()  # ... and a correct one right after it
    assert searches() == before
    same(few, score_matrix(q, db), "the rows searched")
    assert got[7].tobytes() == few[0].tobytes()
    t.close()


def test_stats():
    db, left = data(*K1024)
    t, lt = table(db), table(left)
    for kw, nl, nr in ((dict(), NL, N), (dict(row_begin=7, row_end=9), 2, N), (dict(col_begin=13, col_end=14), NL, 1),
                       (dict(row_begin=1, row_end=130, col_begin=100, col_end=400), 129, 300)):
        st = {}
        out = t.scores(lt, stats=st, **kw)
        assert out.shape == (nl, nr)
        assert st["left_rows"] == nl and st["right_rows"] == nr and st["pairs"] == nl * nr, (kw, st)
        assert st["launches"] == 1 and st["slabs"] == 1, (kw, st)
        assert st["wall_ms"] > 0 and st["kernel_ms"] > 0 and st["prepare_ms"] > 0 and st["d2h_ms"] > 0 and st["clock_mhz"] > 100, (kw, st)
    st = {}
    t.scores(left[:17], col_end=40, stats=st)
    assert (st["left_rows"], st["right_rows"], st["pairs"]) == (17, 40, 680), st
    st = {}
    assert t.scores(lt, row_begin=4, row_end=4, stats=st).shape == (0, N)
    assert st["left_rows"] == 0 and st["right_rows"] == N and st["pairs"] == 0 and st["launches"] == 0 and st["slabs"] == 0, st
    t.close()
    lt.close()
