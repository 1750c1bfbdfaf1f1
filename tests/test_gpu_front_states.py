"""The shared fronts of the two-table calls (capi_front.h) on the GPU: the state errors that need a finalized table, and the three
ways a call takes its left rows.

Folded tables: each of the nine fronts refuses a folded table as `db`, and the four handle fronts (five with the device output)
refuse it as `left`, with GSIM_ERR_STATE, a message that says "folded" and names the side, and `*out` cleared where there is one.
Left-handling forms: on an unfolded pair each family gives the same bytes for left == db, for a second handle that holds the same
rows and for the same rows uploaded as queries, at nl = 300 (one full 256-row owner tile and one of 44 rows) -- at 1024 bits, where
the rows are used as they lie (WP == W), and at 160 bits, where the tile routes read a zero-padded copy and left == db reuses the
table's.  The results are not empty: asserted.  Two devices: the "different devices" message, on two GPUs or, on one, in a child
process on the test-hooks build with two logical devices on GPU 0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = -5
N = 300
EDGES = np.array([0.1, 0.2, 0.3, 0.5, 1.0], np.float32)
FP, U32P, U64P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
GARBAGE = 0xDEAD0


def rows(bits, n=N, seed=0xF207):
    """n rows of `bits` bits, about a quarter of them set; rows 40 and 41 are copies of row 7, row 150 is all-zero."""
    rng = np.random.default_rng(seed + bits)
    db = np.packbits(rng.random((n, bits)) < 0.25, axis=1, bitorder="little").view(np.uint32).copy()
    db[40] = db[41] = db[7]
    db[150] = 0
    return db


def message():
    return capi.load().gsim_last_error().decode()


def fronts(t, left, q):
    """name -> (a call of the front on table t with the left handle `left` or the queries q, has it `out`?)"""
    L = capi.load()
    n, nq = t.count(), len(q)
    nl = left.count()
    qp = q.ctypes.data_as(U32P)
    ep = EDGES.ctypes.data_as(FP)
    hist, total = np.zeros((max(nl, nq), len(EDGES) + 1), np.uint64), np.zeros(len(EDGES) + 1, np.uint64)
    hp, tp = hist.ctypes.data_as(U64P), total.ctypes.data_as(U64P)
    buf = np.zeros(max(nl, nq) * n, np.float32)
    bp = buf.ctypes.data_as(FP)
    keep = (hist, total, buf)
    return {
        "join": (lambda o: L.gsim_db_join(t._h, left._h, 0, nl, 0.5, 0, 1.0, 1.0, 0, o), True, keep),
        "join_queries": (lambda o: L.gsim_db_join_queries(t._h, qp, nq, 0.5, 0, 1.0, 1.0, 0, o), True, keep),
        "knn_join": (lambda o: L.gsim_db_knn_join(t._h, left._h, 0, nl, 5, 0.5, 0, 1.0, 1.0, 0, o), True, keep),
        "knn_queries": (lambda o: L.gsim_db_knn_queries(t._h, qp, nq, 5, 0.5, 0, 1.0, 1.0, o), True, keep),
        "histogram": (lambda o: L.gsim_db_histogram(t._h, left._h, 0, nl, ep, len(EDGES), 0, 1.0, 1.0, 0, hp, tp, None), False, keep),
        "histogram_queries": (lambda o: L.gsim_db_histogram_queries(t._h, qp, nq, ep, len(EDGES), 0, 1.0, 1.0, hp, tp, None), False, keep),
        "scores": (lambda o: L.gsim_db_scores(t._h, left._h, 0, nl, 0, n, 0, 1.0, 1.0, bp, n, None), False, keep),
        "scores_device": (lambda o: L.gsim_db_scores_device(t._h, left._h, 0, nl, 0, n, 0, 1.0, 1.0, C.cast(bp, C.c_void_p), n, None), False, keep),
        "scores_queries": (lambda o: L.gsim_db_scores_queries(t._h, qp, nq, 0, n, 0, 1.0, 1.0, bp, n, None), False, keep),
    }


def refused(call, has_out, word, side):
    g = C.c_void_p(GARBAGE)
    assert call(C.byref(g)) == STATE, message()
    m = message()
    assert word in m, m
    if side is not None:
        assert m.endswith(": " + side), m
    if has_out:
        assert g.value is None, "*out is cleared"


def test_folded_tables_are_a_state_error_on_either_side():
    db = rows(1024)
    plain = capi.Table(1024).add_rows(db).finalize(0, 1)
    folded = capi.Table(1024).add_rows(db).set_fold_factor(2).finalize(0, 1)
    assert folded.fold_factor() == 2 and plain.fold_factor() == 1
    q = db[:7].copy()
    as_db = fronts(folded, plain, q)
    assert len(as_db) == 9
    for name, (call, has_out, _) in as_db.items():
        refused(call, has_out, "folded", "table")
    as_left = fronts(plain, folded, q)
    handle = [name for name in as_left if not name.endswith("queries")]
    assert handle == ["join", "knn_join", "histogram", "scores", "scores_device"]
    for name in handle:
        call, has_out, _ = as_left[name]
        refused(call, has_out, "folded", "left table")
    # both sides the one folded handle: the table is named
    for name, (call, has_out, _) in fronts(folded, folded, q).items():
        refused(call, has_out, "folded", "table")
    plain.close()
    folded.close()


@pytest.mark.parametrize("bits", [1024, 160])
def test_the_three_forms_of_the_left_side_give_the_same_bytes(bits):
    import torch
    db = rows(bits)
    t = capi.Table(bits).add_rows(db).finalize(0, 1)
    twin = capi.Table(bits).add_rows(db).finalize(0, 1)
    assert t.count() == twin.count() == N

    def blob(x):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in x)

    def device_scores(left):
        out = torch.zeros((N, N), dtype=torch.float32, device="cuda:0")
        assert t.scores(left, out_ptr=out.data_ptr()) is None
        return out.cpu().numpy()

    families = {
        "join": lambda left, **kw: t.join(left, 0.14, **kw),
        "join by score": lambda left, **kw: t.join(left, 0.14, order=capi.JOIN_BY_SCORE, **kw),
        "knn join": lambda left, **kw: t.knn_join(left, 5, 0.1, **kw),
        "histogram": lambda left, **kw: t.histogram(left, EDGES, **kw),
        "scores": lambda left, **kw: (t.scores(left, **kw),),
    }
    for name, call in families.items():
        # all 300 rows, and the rows [41, 300): 259 of them, from an odd first row
        for lo in (0, 41):
            same, other, uploaded = call(t, row_begin=lo), call(twin, row_begin=lo), call(db[lo:])
            assert blob(same) == blob(other), (name, lo, "left == db against a second handle")
            assert blob(same) == blob(uploaded), (name, lo, "left == db against uploaded queries")
            assert len(blob(same)) > 0
    assert device_scores(t).tobytes() == device_scores(twin).tobytes() == t.scores(db).tobytes()
    # not vacuous: lists with entries beyond the row itself, counts in several bins, the planted rows
    indptr, indices, scores = t.join(t, 0.14)
    assert len(indptr) == N + 1 and len(indices) > 2 * N and indptr[151] == indptr[150], "the all-zero row lists nothing"
    assert {7, 40, 41} <= set(indices[int(indptr[7]):int(indptr[8])].tolist())
    indptr, indices, scores = t.knn_join(db, 5, 0.1)
    assert int(indptr[-1]) == 5 * (N - 1) and indices[int(indptr[40]):int(indptr[40]) + 3].tolist() == [7, 40, 41]
    hist, total = t.histogram(twin, EDGES)
    assert int(hist.sum()) == N * N and (total > 0).sum() >= 3 and int(total[-1]) >= N - 1 + 6
    S = t.scores(twin)
    assert S.shape == (N, N) and S[7, 41] == 1.0 and S[150, 0] == 0.0 and S[150, 150] == 0.0 and (np.diag(S)[:150] == 1.0).all()
    # the streaming routes take the same three forms (a left side of two rows, of which the second is not the table's first)
    st, hs = {}, {}
    a, b, c = t.join(t, 0.14, row_begin=6, row_end=8, stats=st), t.join(twin, 0.14, row_begin=6, row_end=8), t.join(db[6:8], 0.14)
    assert st["rows_streamed"] == 2 and blob(a) == blob(b) == blob(c) and {7, 40, 41} <= set(a[1].tolist())
    a, b, c = t.histogram(t, EDGES, row_begin=6, row_end=8, stats=hs), t.histogram(twin, EDGES, row_begin=6, row_end=8), t.histogram(db[6:8], EDGES)
    assert hs["rows_streamed"] == 2 and blob(a) == blob(b) == blob(c) and int(a[1].sum()) == 2 * N
    t.close()
    twin.close()


def two_handles_on_two_devices():
    db = rows(1024)
    a, b = capi.Table(1024).add_rows(db).finalize(0, 1), capi.Table(1024).add_rows(db).finalize(1, 1)
    for name, (call, has_out, _) in fronts(a, b, db[:3].copy()).items():
        if name.endswith("queries"):
            continue
        refused(call, has_out, "the two handles are on different devices", None)
    a.close()
    b.close()


def test_handles_on_two_devices_are_a_state_error():
    """Fewer than two GPUs: the same test in a child process on the test-hooks build with two logical devices on GPU 0."""
    if capi.device_count() >= 2:
        return two_handles_on_two_devices()
    from conftest import hooks_env
    assert not os.environ.get("GSIM_TEST_ALIAS_DEVICES"), "two logical devices asked for, %d seen" % capi.device_count()
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_handles_on_two_devices_are_a_state_error"], env=hooks_env(GSIM_TEST_ALIAS_DEVICES="2"), capture_output=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0 and b"1 passed" in p.stdout, p.stdout.decode("utf-8", "replace")[-3000:]
