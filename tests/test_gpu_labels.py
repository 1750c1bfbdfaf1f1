"""The column counts of every label in one pass on the GPU (gsim_db_label_counts).

Expected values: tests/kmeans_rule.py (np.unpackbits, sums per label).  Everything is an integer and compared exactly.

Data: tables of N = 5000 rows synth_rows(31, kind, 0, N, W) with an all-zero and an all-ones row.  Label vectors: uniform over 7 and
over 1000 labels; skewed (one label with 90 % of the rows plus 400 singletons); every row its own label; 6000 labels, so that empty
ones exist; 10 % of the rows GSIM_LABEL_NONE; a single label.  Between them segments far longer than a step of the counting kernel
(its LDS counters), segments of a row or two (its global adds) and both in one call.  Asserted on the EXPECTED sizes: an empty label,
a singleton and a label above 4000 rows appear across the cases."""
import contextlib
import os

import numpy as np
import pytest

import kmeans_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
ROWS = "GSIM_LABELS_LAUNCH_ROWS"
N = 5000
NONE = capi.LABEL_NONE


@contextlib.contextmanager
def knob(value):
    old = os.environ.get(ROWS)
    if value is None:
        os.environ.pop(ROWS, None)
    else:
        os.environ[ROWS] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ROWS, None)
        else:
            os.environ[ROWS] = old


def table(db, rows=None):
    with knob(rows):  # (read once per handle, by gsim_db_create)
        return capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)


_data = {}


def data(kind, W):
    if (kind, W) not in _data:
        db = O.synth_rows(31, kind, 0, N, W)
        db[2500] = 0
        db[2501] = 0xFFFFFFFF
        db.setflags(write=False)
        _data[(kind, W)] = db
    return _data[(kind, W)]


def label_vectors():
    """-> {name: (labels, nlabels)}; the same for every table"""
    rng = np.random.default_rng(5)
    out = {}
    out["uniform 7"] = (rng.integers(0, 7, N), 7)
    out["uniform 1000"] = (rng.integers(0, 1000, N), 1000)
    skew = np.zeros(N, np.int64)
    singles = rng.choice(N, 400, replace=False)
    skew[singles] = 1 + np.arange(400)
    skew[rng.choice(np.setdiff1d(np.arange(N), singles), 100, replace=False)] = 401
    out["skewed"] = (skew, 402)
    out["every row its own"] = (rng.permutation(N), N)
    out["6000 labels"] = (rng.integers(0, 6000, N), 6000)
    none = rng.integers(0, 50, N)
    none[rng.choice(N, N // 10, replace=False)] = NONE
    out["a tenth nowhere"] = (none, 50)
    out["one label"] = (np.zeros(N, np.int64), 1)
    return {k: (v.astype(np.uint32), L) for k, (v, L) in out.items()}


LABELS = label_vectors()


def test_the_label_vectors_cover_the_cases():
    sizes = {k: np.bincount(v[v != NONE], minlength=L) for k, (v, L) in LABELS.items()}
    assert any((s == 0).any() for s in sizes.values()), "an empty label"
    assert any((s == 1).any() for s in sizes.values()), "a singleton"
    assert any((s > 4000).any() for s in sizes.values()), "a label above 4000 rows"
    assert sizes["skewed"][0] == 4500 and (sizes["skewed"][1:401] == 1).all() and sizes["skewed"][401] == 100
    assert (sizes["every row its own"] == 1).all() and (sizes["6000 labels"] == 0).sum() > 1000
    assert (LABELS["a tenth nowhere"][0] == NONE).sum() == N // 10 and sizes["one label"].tolist() == [N]


@pytest.mark.parametrize("bits", [32, 96, 160, 1024, 2080, 4096])
@pytest.mark.parametrize("kind", [O.KIND_MORGAN, O.KIND_DENSE])
def test_parity_with_numpy(bits, kind):
    """Rows of whole 16-byte chunks (32 ... 4096 bits: 1024, 4096) and the word-granular variant (32, 96, 160, 2080)."""
    W = bits // 32
    db = data(kind, W)
    t = table(db)
    for name, (labels, L) in LABELS.items():
        want_c, want_s = R.label_counts(db, labels, L)
        assert int(want_s.sum()) == int((labels != NONE).sum()) and want_c[:, :].max() <= want_s.max()
        st = {}
        got_c, got_s = t.label_counts(labels, L, stats=st)
        assert got_c.dtype == np.uint32 and got_c.shape == (L, bits) and got_s.dtype == np.uint32
        assert np.array_equal(got_s, want_s), (bits, kind, name)
        bad = np.argwhere(got_c != want_c)
        assert len(bad) == 0, (bits, kind, name, len(bad), bad[:5].tolist())
        assert st["rows_read"] == N and st["rows_counted"] == int(want_s.sum()) and st["labels"] == L and st["launches"] >= 1, st
    t.close()


def test_rows_of_the_result_equal_bit_counts_of_the_row_sets():
    db = data(O.KIND_MORGAN, 32)
    t = table(db)
    for name in ("uniform 7", "skewed", "a tenth nowhere"):
        labels, L = LABELS[name]
        counts, sizes = t.label_counts(labels, L)
        for l in (0, L // 2, L - 1):
            rows = np.flatnonzero(labels == l).astype(np.uint32)
            rs = t.rowset(rows=rows)
            c, n = t.bit_counts(rowset=rs)
            assert n == sizes[l] == len(rows) and np.array_equal(c, counts[l].astype(np.uint64)), (name, l)
            rs.close()
    t.close()


@pytest.mark.parametrize("bits", [1024, 160])
def test_ranges_add_up_and_launch_cuts_change_nothing(bits):
    db = data(O.KIND_MORGAN, bits // 32)
    t = table(db)
    cut = table(db, rows=300)
    for name in ("uniform 1000", "skewed", "a tenth nowhere"):
        labels, L = LABELS[name]
        st0, st = {}, {}
        whole_c, whole_s = t.label_counts(labels, L, stats=st0)
        assert np.array_equal(whole_c, R.label_counts(db, labels, L)[0])
        parts = [t.label_counts(labels[a:b], L, row_begin=a, row_end=b) for a, b in ((0, 1), (1, 1777), (1777, 1777), (1777, N))]
        assert np.array_equal(sum(p[0].astype(np.uint64) for p in parts), whole_c) and np.array_equal(sum(p[1].astype(np.uint64) for p in parts), whole_s)
        assert not parts[2][0].any() and not parts[2][1].any(), "an empty range: zeros"
        got_c, got_s = cut.label_counts(labels, L, stats=st)
        assert st0["launches"] == 1 and st["launches"] == (st["rows_counted"] + 299) // 300 > 10, (st0, st)
        assert got_c.tobytes() == whole_c.tobytes() and got_s.tobytes() == whole_s.tobytes(), name
        again = t.label_counts(labels, L)
        assert again[0].tobytes() == whole_c.tobytes(), "a second call"
    t.set_row_base(1000)
    labels, L = LABELS["uniform 7"]
    assert np.array_equal(t.label_counts(labels[10:900], L, row_begin=10, row_end=900)[0], R.label_counts(db[10:900], labels[10:900], L)[0]), "no row base"
    t.close()
    cut.close()


def test_the_labels_of_leader_and_maxmin_go_in_unchanged():
    db = data(O.KIND_MORGAN, 32)
    t = table(db)
    leaders, leader_of, _, _ = t.leader(0.6, max_leaders=40)
    assert (leader_of == capi.LEADER_NONE).any() and len(leaders) == 40, "the cap leaves rows unassigned: LEADER_NONE == LABEL_NONE"
    counts, sizes = t.label_counts(leader_of, len(leaders))
    want_c, want_s = R.label_counts(db, leader_of, len(leaders))
    assert np.array_equal(counts, want_c) and np.array_equal(sizes, want_s) and int(sizes.sum()) == int((leader_of != NONE).sum())
    picks, _, _, nearest = t.maxmin(25, assign=True)
    counts, sizes = t.label_counts(nearest, len(picks))
    want_c, want_s = R.label_counts(db, nearest, len(picks))
    assert np.array_equal(counts, want_c) and np.array_equal(sizes, want_s) and int(sizes.sum()) == N
    # ... and on to the centroids and the tightness of every cluster
    cen = capi.label_centroids(counts, sizes)
    assert np.array_equal(cen, R.centroids(want_c, want_s))
    tight = [capi.isim(counts[l].astype(np.uint64), int(sizes[l])) for l in range(len(picks))]
    assert all(0.0 <= x <= 1.0 for x in tight)
    t.close()


def test_generated_and_attached_tables_and_the_search_state():
    import torch
    W, seed = 5, 0xB0B
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, N, W)
    labels, L = LABELS["skewed"]
    want = R.label_counts(db, labels, L)
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, N, 0)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), N, 0)
    for x in (g, a):
        got = x.label_counts(labels, L)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        x.close()
    del ten
    db = data(O.KIND_MORGAN, 32)
    t = table(db)
    t.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 1500, 4999]])

    def searches():
        hits, approx = t.search(q, 50, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0 = t.timing()
    got = t.label_counts(*LABELS["uniform 1000"])
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    bad = LABELS["uniform 7"][0].copy()
    bad[17] = 7
    with pytest.raises(capi.GsimError) as e:
        t.label_counts(bad, 7)  # a failed call ...
    assert e.value.code == -1
    assert t.label_counts(*LABELS["uniform 1000"])[0].tobytes() == got[0].tobytes()  # ... and a correct one right after it
    assert searches() == before
    t.close()
