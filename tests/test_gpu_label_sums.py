"""Quantised score sums by label on the GPU (gsim_db_label_sums), and the silhouettes and medoids made of them.

Expected values: tests/label_sums_rule.py over the oracle's f32 scores.  Everything is an integer and compared exactly.

Data: tables of N = 3000 rows synth_rows(31, kind, 0, N, W), i.i.d. and Morgan-shaped, W of 4, 5, 32, 48, 64 and 128 words (every
padded width of the kernel), with fixed rows: an all-zero row, an all-ones row, three identical rows (in a labelling that gives them
different labels their means are equal: a label tie) and, where a row has 771 bits, a row with one bit set and a row with 771 bits
set that contains it -- their score 1 / 771 has an ulp below 2^-31, so the truncation acts.  Label vectors as
tests/test_gpu_labels.py's, for N = 3000: uniform over 7 and over 1000 labels; skewed (one label of 2500 rows, 400 singletons, one
of 100); every row its own label; twice as many labels as rows; a tenth of the rows GSIM_LABEL_NONE; a single label.
What the data has to provide is asserted on the EXPECTED values (test_the_data_provide_the_cases)."""
import numpy as np
import pytest

import label_sums_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
N = 3000
NONE = capi.LABEL_NONE
TAN = {}
TV55 = dict(metric=capi.METRIC_TVERSKY, alpha=np.float32(0.5), beta=np.float32(0.5))
TV37 = dict(metric=capi.METRIC_TVERSKY, alpha=np.float32(0.3), beta=np.float32(0.7))
METRICS = {"tanimoto": TAN, "tversky 0.5 0.5": TV55, "tversky 0.3 0.7": TV37}
MAIN = (O.KIND_MORGAN, 32)
# every padded width, both kinds; the main table under every metric, one narrow table under Tversky too
TABLES = [(O.KIND_DENSE, 4), (O.KIND_MORGAN, 5), (O.KIND_DENSE, 32), MAIN, (O.KIND_MORGAN, 48), (O.KIND_DENSE, 64), (O.KIND_MORGAN, 128)]
CASES = [(k, W, "tanimoto") for k, W in TABLES] + [(k, W, m) for k, W in (MAIN, (O.KIND_MORGAN, 5)) for m in ("tversky 0.5 0.5", "tversky 0.3 0.7")]
ZERO, ONES, SAME, ONE_BIT, MANY_BITS = 0, 1, (2, 3, 4), 5, 6

_data, _scores, _want = {}, {}, {}


def data(kind, W):
    if (kind, W) not in _data:
        db = O.synth_rows(31, kind, 0, N, W)
        db[ZERO] = 0
        db[ONES] = 0xFFFFFFFF
        for r in SAME:
            db[r] = db[10]
        if W * 32 >= 771:
            db[ONE_BIT] = 0
            db[ONE_BIT, 0] = 1 << 3
            db[MANY_BITS] = 0
            db[MANY_BITS, :24] = 0xFFFFFFFF
            db[MANY_BITS, 24] = 7
        db.setflags(write=False)
        _data[(kind, W)] = db
    return _data[(kind, W)]


def scores(kind, W, metric):
    if (kind, W, metric) not in _scores:
        S = R.score_matrix(data(kind, W), METRICS[metric])
        S.setflags(write=False)
        _scores[(kind, W, metric)] = S
    return _scores[(kind, W, metric)]


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


def names_for(kind, W, metric):
    return list(LABELS) if (kind, W) == MAIN and metric == "tanimoto" else ["skewed", "a tenth nowhere"]


def want(kind, W, metric, name, lo=0, hi=N):
    """the rule's (own_q, other_label, other_q, sizes, ties) of the rows [lo, hi): computed once, never modified"""
    key = (kind, W, metric, name, lo, hi)
    if key not in _want:
        labels, nlabels = LABELS[name]
        _want[key] = R.sums(scores(kind, W, metric)[lo:hi, lo:hi], labels[lo:hi], nlabels)
        for x in _want[key][:4]:
            x.setflags(write=False)
    return _want[key]


def table(db, row_base=0):
    t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if row_base:
        t.set_row_base(row_base)
    return t


@pytest.fixture(scope="module")
def main_table():
    t = table(data(*MAIN))
    yield t
    t.close()


def same(got, w, what):
    own, other, other_q, sizes, _ = got
    assert np.array_equal(sizes, w[3]), what
    assert np.array_equal(own, w[0]), (what, np.flatnonzero(own != w[0])[:10])
    assert np.array_equal(other, w[1]), (what, np.flatnonzero(other != w[1])[:10])
    assert np.array_equal(other_q, w[2]), (what, np.flatnonzero(other_q != w[2])[:10])


def test_the_data_provide_the_cases():
    S = scores(*MAIN, "tanimoto")
    assert R.inexact(S).any(), "some pair has an s * 2^31 that is not an integer"
    assert R.inexact(S[ONE_BIT, MANY_BITS]) and S[ONE_BIT, MANY_BITS] == np.float32(1.0) / np.float32(771.0)
    assert S[ZERO].max() == 0.0 and S[SAME[0], SAME[1]] == 1.0
    own, other, other_q, sizes, ties = want(*MAIN, "tanimoto", "every row its own")
    assert len(ties) > 0 and set(SAME) <= set(ties), "some row's best mean is shared by two labels"
    assert other[SAME[0]] == min(LABELS["every row its own"][0][[SAME[1], SAME[2], 10]]), "the lowest of the tied labels"
    assert (want(*MAIN, "tanimoto", "one label")[1] == NONE).all(), "rows without another cluster"
    assert (want(*MAIN, "tanimoto", "a tenth nowhere")[1] == NONE).sum() == N // 10
    z = [want(*MAIN, "tanimoto", name)[3] for name in LABELS]
    assert any((s == 0).any() for s in z) and any((s == 1).any() for s in z) and any((s > 2400).any() for s in z)
    assert z[2][0] == 2500 and (z[2][1:401] == 1).all() and z[2][401] == 100


@pytest.mark.parametrize("kind,W,metric", CASES)
def test_sums_match_the_rule(kind, W, metric):
    t = table(data(kind, W))
    try:
        for name in names_for(kind, W, metric):
            labels, nlabels = LABELS[name]
            w = want(kind, W, metric, name)
            got = t.label_sums(labels, nlabels, **METRICS[metric])
            same(got, w, (W, metric, name))
            st = got[4]
            nlab = int((labels != NONE).sum())
            assert st["rows"] == N and st["rows_labelled"] == nlab and st["labels_nonempty"] == int((w[3] > 0).sum())
            assert st["pairs"] == nlab * nlab - nlab and st["launches"] >= 1
            # the medoid route: only own_q and sizes, and only the pairs inside a cluster
            own, other, other_q, sizes, st = t.label_sums(labels, nlabels, own_only=True, **METRICS[metric])
            assert other is None and other_q is None
            assert np.array_equal(own, w[0]) and np.array_equal(sizes, w[3]), (W, metric, name)
            assert st["pairs"] == int((w[3].astype(np.int64) ** 2).sum()) - nlab
    finally:
        t.close()


@pytest.mark.parametrize("name", ["skewed", "uniform 1000", "a tenth nowhere"])
def test_a_sub_range_and_a_row_base(name, main_table):
    labels, nlabels = LABELS[name]
    lo, hi = 700, 2300
    w = want(*MAIN, "tanimoto", name, lo, hi)
    got = main_table.label_sums(labels[lo:hi], nlabels, lo, hi)
    same(got, w, name)
    assert got[4]["rows"] == hi - lo
    own = main_table.label_sums(labels[lo:hi], nlabels, lo, hi, own_only=True)[0]
    assert np.array_equal(own, w[0])
    based = table(data(*MAIN), row_base=1 << 20)
    try:
        same(based.label_sums(labels[lo:hi], nlabels, lo, hi), w, name)
        same(based.label_sums(labels, nlabels), want(*MAIN, "tanimoto", name), name)
    finally:
        based.close()
    # an empty range: GSIM_OK, zeroed sizes
    own, other, other_q, sizes, st = main_table.label_sums([], nlabels, 5, 5)
    assert len(own) == 0 and len(other) == 0 and not sizes.any() and st["launches"] == 0


@pytest.mark.parametrize("name", ["skewed", "uniform 7", "every row its own"])
def test_the_launch_cut_and_the_run_change_nothing(name, main_table):
    labels, nlabels = LABELS[name]
    w = want(*MAIN, "tanimoto", name)
    for own_only in (False, True):
        whole = main_table.label_sums(labels, nlabels, own_only=own_only)
        cut = main_table.label_sums(labels, nlabels, own_only=own_only, launch_pairs=64 * 256)  # pieces of 256 candidates: inside long segments
        again = main_table.label_sums(labels, nlabels, own_only=own_only)
        for got in (whole, cut, again):
            assert got[0].tobytes() == w[0].tobytes() and got[3].tobytes() == w[3].tobytes()
            if not own_only:
                assert got[1].tobytes() == w[1].tobytes() and got[2].tobytes() == w[2].tobytes()
        if not own_only or name != "every row its own":
            assert cut[4]["launches"] > whole[4]["launches"] >= 1, (name, own_only, cut[4]["launches"], whole[4]["launches"])
        assert again[4]["launches"] == whole[4]["launches"]


@pytest.mark.parametrize("name", ["uniform 7", "skewed", "a tenth nowhere", "every row its own", "one label"])
def test_silhouettes_and_medoids_from_the_gpu_sums(name, main_table):
    labels, nlabels = LABELS[name]
    w = want(*MAIN, "tanimoto", name)
    own, other, other_q, sizes, _ = main_table.label_sums(labels, nlabels)
    sil, lmean, mean = capi.label_silhouette(labels, own, other, other_q, sizes)
    wsil, wlmean, wmean = R.silhouette(labels, w[0], w[1], w[2], w[3])
    assert sil.view(np.uint64).tobytes() == wsil.view(np.uint64).tobytes()
    assert lmean.view(np.uint64).tobytes() == wlmean.view(np.uint64).tobytes() and np.float64(mean).tobytes() == np.float64(wmean).tobytes()
    assert float(np.abs(sil).max()) <= 1.0
    med = capi.label_medoids(labels, main_table.label_sums(labels, nlabels, own_only=True)[0], nlabels)
    assert np.array_equal(med, R.medoids(labels, w[0], nlabels))
    assert (med[sizes > 0] != NONE).all() and (med[sizes == 0] == NONE).all()


def test_a_search_before_and_after_returns_the_same_hits(main_table):
    db = data(*MAIN)
    q = db[[17, 1234]]
    before = main_table.search(q, 50, 0.1)
    labels, nlabels = LABELS["uniform 1000"]
    main_table.label_sums(labels, nlabels)
    main_table.label_sums(labels, nlabels, own_only=True, launch_pairs=64 * 256)
    after = main_table.search(q, 50, 0.1)
    assert all(b.tobytes() == a.tobytes() for b, a in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    want_hits, _ = O.search(q[0], db, 50, 0.1, nthreads=4)
    assert len(want_hits) > 0 and np.array_equal(after[0][0]["row"], want_hits["row"])
