"""Label-grouped search on the GPU (gsim_db_search_labels): the best hit and the hit count of every label.

Expected values: tests/search_labels_rule.py over the oracle's f32 scores.  Everything is compared exactly: hits as bytes, labels,
counts, approx, rows_kept, label_best as bytes, label_kept.

Data: tables of N = 3000 rows synth_rows(31, kind, 0, N, W) at W = 4, 5, 32, 48, 64 and 128 words (every specialised width and the
word loop, i.i.d. and Morgan-shaped), and one main table of 20 011 Morgan-shaped 1024-bit rows (not a multiple of 64: several
workgroups hold candidates for the same label and the last chunk is partial).  Fixed rows: an all-zero row, an all-ones row, three
rows identical to row 10 -- "uniform 7" puts them into one label (the tie inside a label: the lowest row), "uniform 1000" into three
(the tie between labels' bests).  Label vectors as tests/test_gpu_label_sums.py's, plus labels in sorted (cluster) order, where every
lane of a wave meets one address, and 40 000 labels on the main table, which fit no LDS budget.
Queries: a pool of 37 -- row 10 (score 1.0 against its duplicates), the all-zero query, table rows and rows of another seed -- of
which the first 1, 5 or 37 are asked (37: two full tiles and a remainder).
Cutoffs: 0, negative, 2^-20 (dense), one taken from the expected values so that between a quarter and three quarters of the labels
keep a row, 1.0 and 1.5.  What the data has to provide is asserted on the EXPECTED values (test_the_data_provide_the_cases)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import search_labels_rule as R
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
NONE = capi.LABEL_NONE
TAN = {}
TV37 = dict(metric=capi.METRIC_TVERSKY, alpha=np.float32(0.3), beta=np.float32(0.7))
METRICS = {"tanimoto": TAN, "tversky 0.3 0.7": TV37}
N_SMALL, N_MAIN = 3000, 20011
MAIN = (O.KIND_MORGAN, 32, N_MAIN)
SMALL = [(O.KIND_DENSE, 4), (O.KIND_MORGAN, 5), (O.KIND_DENSE, 32), (O.KIND_MORGAN, 32), (O.KIND_MORGAN, 48), (O.KIND_DENSE, 64), (O.KIND_MORGAN, 128)]
ZERO, ONES, SAME, TWIN = 0, 1, (2, 3, 4), 10
NQ = 37
LDS_BUDGET = 144 * 1024  # include/gpusim_hip.h: route LDS while one query's nlabels x 8 (12 when counting) bytes fit 144 KiB
DENSE = 2.0 ** -20

_data, _queries, _hits = {}, {}, {}


def data(kind, W, n):
    if (kind, W, n) not in _data:
        db = O.synth_rows(31, kind, 0, n, W)
        db[ZERO] = 0
        db[ONES] = 0xFFFFFFFF
        for r in SAME:
            db[r] = db[TWIN]
        db.setflags(write=False)
        _data[(kind, W, n)] = db
    return _data[(kind, W, n)]


def queries(kind, W, n):
    """the pool: row 10, the all-zero query, then table rows and rows the table does not hold"""
    if (kind, W, n) not in _queries:
        db = data(kind, W, n)
        q = np.concatenate([db[[TWIN]], np.zeros((1, W), np.uint32), db[[17, n - 1, ONES]], O.synth_rows(77, kind, 0, 16, W),
                            db[(np.arange(16) * 173 + 29) % n]])
        assert len(q) == NQ
        q.setflags(write=False)
        _queries[(kind, W, n)] = q
    return _queries[(kind, W, n)]


def pair_hits(kind, W, n, metric, nq):
    """the rule's input for the first nq queries of the pool: computed once, never modified"""
    key = (kind, W, n, metric)
    if key not in _hits or len(_hits[key]) < nq:
        H = R.pair_hits(data(kind, W, n), queries(kind, W, n)[:nq], METRICS[metric])
        H.setflags(write=False)
        _hits[key] = H
    return _hits[key][:nq]


def label_vectors(n):
    """-> {name: (labels, nlabels)}"""
    rng = np.random.default_rng(5)
    out = {}
    u7 = rng.integers(0, 7, n)
    u7[list(SAME)] = 3
    out["uniform 7"] = (u7, 7)
    u1000 = rng.integers(0, 1000, n)
    u1000[list(SAME)] = (10, 11, 12)
    out["uniform 1000"] = (u1000, 1000)
    skew = np.zeros(n, np.int64)
    singles = rng.choice(n, 400, replace=False)
    skew[singles] = 1 + np.arange(400)
    skew[rng.choice(np.setdiff1d(np.arange(n), singles), 100, replace=False)] = 401
    out["skewed"] = (skew, 402)
    out["every row its own"] = (rng.permutation(n), n)
    out["twice as many labels"] = (rng.integers(0, 2 * n, n), 2 * n)
    none = rng.integers(0, 50, n)
    none[rng.choice(n, n // 10, replace=False)] = NONE
    out["a tenth nowhere"] = (none, 50)
    out["one label"] = (np.zeros(n, np.int64), 1)
    out["cluster order"] = (np.sort(rng.integers(0, 300, n)), 300)
    if n == N_MAIN:
        out["40000 labels"] = (rng.integers(0, 40000, n), 40000)
    return {k: (v.astype(np.uint32), L) for k, (v, L) in out.items()}


LABELS = {N_SMALL: label_vectors(N_SMALL), N_MAIN: label_vectors(N_MAIN)}


def selective_cutoff(H, labels, nlabels):
    """from the expected values: the median of the labels' best scores for query 2 of the pool (table row 17) -- about half of the
    labels keep a row; asserted by the callers"""
    w = R.one_query(H[2], labels, nlabels, 0, 0.0)
    best = w["label_best"]["score"][w["label_kept"] > 0]
    return float(np.median(best[best > 0]))


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


def check_route(st, nlabels, cutoff, what):
    """the route the header states, from the call's stats"""
    cell = 12 if cutoff > 0 else 8  # (the callers ask for the per-label outputs: rows are counted under a cutoff)
    lds = nlabels * cell <= LDS_BUDGET
    assert st["passes"] >= 1 and st["passes"] == st["passes_lds"] + st["passes_global"], what
    assert (st["passes_lds"] > 0) == lds and (st["passes_global"] > 0) == (not lds), (what, st)


def test_the_data_provide_the_cases():
    H = pair_hits(*MAIN, "tanimoto", NQ)
    S = H["score"]
    assert (S[0, [TWIN, *SAME]] == 1.0).all() and (S[0] == 1.0).sum() == 4, "row 10 and its three copies, nothing else"
    assert S[1].max() == 0.0 and S[:, ZERO].max() == 0.0, "all-zero scores: the all-zero query, the all-zero row"
    lab = LABELS[N_MAIN]
    w = R.one_query(H[0], *lab["uniform 7"], 7, 0.0)
    assert w["label_best"][3]["row"] == SAME[0] and w["label_kept"][3] > 3, "the tie inside a label: the lowest row"
    w = R.one_query(H[0], *lab["uniform 1000"], 1000, 0.0)
    assert [int(x) for x in w["hit_labels"][:3]] == [10, 11, 12] and (w["hits"]["score"][:4] == 1.0).all(), "the tie between labels' bests: by row"
    assert w["hits"]["row"][:4].tolist() == [2, 3, 4, 10]
    sizes = np.bincount(lab["twice as many labels"][0], minlength=2 * N_MAIN)
    assert (sizes == 0).sum() > N_MAIN and (np.bincount(lab["40000 labels"][0], minlength=40000) == 0).any(), "empty labels"
    labels, nlabels = lab["uniform 1000"]
    sel = selective_cutoff(H[:5], labels, nlabels)
    w = R.one_query(H[2], labels, nlabels, 0, sel)
    assert nlabels / 4 <= w["approx"] <= 3 * nlabels / 4, "labels without a kept row, and with one"
    assert ((w["label_kept"] == 0) & (np.bincount(labels, minlength=nlabels) > 0)).any()
    w = R.one_query(H[0], labels, nlabels, 5, 1.0)
    assert w["approx"] == 4 and w["rows_kept"] == 4, "cutoff 1.0: exact duplicates only"
    assert R.one_query(H[0], labels, nlabels, 5, 1.5)["approx"] == 0 and R.one_query(H[1], labels, nlabels, 5, DENSE)["approx"] == 0
    w = R.one_query(H[2], labels, nlabels, 1000, 0.0)
    ties = np.flatnonzero(np.diff(w["hits"]["score"]) == 0)
    assert len(ties) > 0, "ties between labels' bests on an ordinary query"
    assert 0 < R.one_query(H[2], labels, nlabels, 0, DENSE)["rows_kept"] < N_MAIN, "the dense cutoff drops the rows that share no bit"


# every width under Tanimoto; Tversky on one word-loop width and one register width
WIDTH_CASES = [(k, W, "tanimoto") for k, W in SMALL] + [(O.KIND_MORGAN, W, "tversky 0.3 0.7") for W in (5, 32)]


@pytest.mark.parametrize("kind,W,metric", WIDTH_CASES)
def test_every_width_matches_the_rule(kind, W, metric):
    n = N_SMALL
    H = pair_hits(kind, W, n, metric, 5)
    t = table(data(kind, W, n))
    try:
        for name in ("skewed", "a tenth nowhere", "twice as many labels", "cluster order"):
            labels, nlabels = LABELS[n][name]
            with t.labelset(labels, nlabels) as ls:
                sizes, labelled, nonempty = ls.sizes()
                assert np.array_equal(sizes, np.bincount(labels[labels != NONE], minlength=nlabels)) and labelled == (labels != NONE).sum()
                assert nonempty == (sizes > 0).sum()
                for cutoff in (0.0, DENSE, selective_cutoff(H, labels, nlabels)):
                    got = t.search_labels(ls, queries(kind, W, n)[:5], 20, cutoff, per_label=True, stats=True, **METRICS[metric])
                    R.same(got, R.expect(H, labels, nlabels, 20, cutoff), (W, metric, name, cutoff))
                    check_route(got["stats"], nlabels, cutoff, (W, name, cutoff))
    finally:
        t.close()


@pytest.mark.parametrize("name", list(LABELS[N_MAIN]))
def test_the_main_table_matches_the_rule(name, main_table):
    labels, nlabels = LABELS[N_MAIN][name]
    q = queries(*MAIN)
    H = pair_hits(*MAIN, "tanimoto", NQ)
    sel = selective_cutoff(H[:5], labels, nlabels)
    kept = R.one_query(H[2], labels, nlabels, 0, sel)["approx"]
    nonempty = int((np.bincount(labels[labels != NONE], minlength=nlabels) > 0).sum())
    assert nonempty / 4 <= kept <= 3 * nonempty / 4 or nonempty == 1, (name, kept, nonempty)
    routes = set()
    with main_table.labelset(labels, nlabels) as ls:
        for cutoff in (0.0, -1.0, DENSE, sel, 1.0, 1.5):
            approx5 = int(R.one_query(H[2], labels, nlabels, 0, cutoff)["approx"])
            for k in sorted({0, 1, max(approx5 // 2, 2), nlabels + 7}):  # none, one, below approx, above nlabels
                got = main_table.search_labels(ls, q[:5], k, cutoff, per_label=True, stats=True)
                R.same(got, R.expect(H[:5], labels, nlabels, k, cutoff), (name, cutoff, k))
                check_route(got["stats"], nlabels, cutoff, (name, cutoff))
                routes.add("lds" if got["stats"]["passes_lds"] else "global")
        for nq in (1, NQ):  # one query; two full tiles and a remainder
            for cutoff in (0.0, sel):
                got = main_table.search_labels(ls, q[:nq], 10, cutoff, per_label=True, stats=True)
                R.same(got, R.expect(H[:nq], labels, nlabels, 10, cutoff), (name, cutoff, nq))
                assert got["stats"]["queries"] == nq and got["stats"]["labels"] == nlabels and got["stats"]["passes"] >= (nq + 15) // 16
    assert routes == ({"global"} if nlabels * 8 > LDS_BUDGET else {"lds"} if nlabels * 12 <= LDS_BUDGET else {"lds", "global"}), (name, routes)


@pytest.mark.parametrize("name", ["uniform 1000", "a tenth nowhere", "40000 labels"])
def test_tversky_on_the_main_table(name, main_table):
    labels, nlabels = LABELS[N_MAIN][name]
    H = pair_hits(*MAIN, "tversky 0.3 0.7", 5)
    with main_table.labelset(labels, nlabels) as ls:
        for cutoff in (0.0, selective_cutoff(H, labels, nlabels), 1.0):
            got = main_table.search_labels(ls, queries(*MAIN)[:5], 50, cutoff, per_label=True, **TV37)
            R.same(got, R.expect(H, labels, nlabels, 50, cutoff), (name, cutoff))


def test_both_routes_were_exercised(main_table):
    q = queries(*MAIN)[:5]
    seen = {}
    for name in ("uniform 1000", "40000 labels"):
        labels, nlabels = LABELS[N_MAIN][name]
        with main_table.labelset(labels, nlabels) as ls:
            seen[name] = main_table.search_labels(ls, q, 10, 0.25, per_label=True, stats=True)["stats"]
    assert seen["uniform 1000"]["passes_lds"] >= 1 and seen["uniform 1000"]["passes_global"] == 0, seen
    assert seen["40000 labels"]["passes_global"] >= 1 and seen["40000 labels"]["passes_lds"] == 0, seen


def test_the_three_identities_on_the_gpu(main_table):
    db = data(*MAIN)
    q = queries(*MAIN)[:5]
    H = pair_hits(*MAIN, "tanimoto", 5)
    sel = selective_cutoff(H, *LABELS[N_MAIN]["uniform 7"])
    # labels[r] = r: gsim_db_search's hits, counts and approx byte for byte, hit_labels = row - row_base
    with main_table.labelset(np.arange(N_MAIN, dtype=np.uint32), N_MAIN) as ls:
        for cutoff in (0.0, DENSE, sel, 1.0):
            for k in (1, 50):
                hits, approx = main_table.search(q, k, cutoff)
                got = main_table.search_labels(ls, q, k, cutoff)
                assert np.array_equal(got["approx"], approx) and np.array_equal(got["rows_kept"], approx), cutoff
                for i in range(5):
                    assert got["counts"][i] == len(hits[i]) and got["hits"][i, :len(hits[i])].tobytes() == hits[i].tobytes(), (cutoff, k, i)
                    assert np.array_equal(got["hit_labels"][i, :len(hits[i])], hits[i]["row"])
    # one label: gsim_db_search at k = 1
    with main_table.labelset(np.zeros(N_MAIN, np.uint32), 1) as ls:
        for cutoff in (0.0, sel, 1.0):
            hits, approx = main_table.search(q, 1, cutoff)
            got = main_table.search_labels(ls, q, 3, cutoff, per_label=True)
            assert np.array_equal(got["rows_kept"], approx) and np.array_equal(got["label_kept"][:, 0], approx.astype(np.uint32))
            for i in range(5):
                assert got["counts"][i] == len(hits[i]) == got["approx"][i] and got["hits"][i, :len(hits[i])].tobytes() == hits[i].tobytes()
    # every label: the hit and the approx of gsim_db_search_rows at k = 1 on the label's rows
    labels, nlabels = LABELS[N_MAIN]["uniform 7"]
    with main_table.labelset(labels, nlabels) as ls:
        for cutoff in (0.0, sel):
            got = main_table.search_labels(ls, q, 7, cutoff, per_label=True)
            for l in range(nlabels):
                rs = main_table.rowset(rows=np.flatnonzero(labels == l).astype(np.uint32))
                hits, approx = main_table.search_rows(rs, q, 1, cutoff)
                rs.close()
                assert np.array_equal(got["label_kept"][:, l], approx.astype(np.uint32)), (cutoff, l)
                for i in range(5):
                    if approx[i]:
                        assert got["label_best"][i, l].tobytes() == hits[i][0].tobytes(), (cutoff, l, i)
                    else:
                        assert got["label_best"][i, l] == R.NO_HIT
    assert db is data(*MAIN)


def test_optional_outputs_null_against_given(main_table):
    L = capi.load()
    labels, nlabels = LABELS[N_MAIN]["skewed"]
    q = np.ascontiguousarray(queries(*MAIN)[:5])
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    with main_table.labelset(labels, nlabels) as ls:
        for cutoff in (0.0, 0.3):
            full = main_table.search_labels(ls, q, 30, cutoff, per_label=True)
            hits = np.zeros((5, 30), capi.HIT_DTYPE)
            hit_labels = np.zeros((5, 30), np.uint32)
            counts = np.zeros(5, np.uint32)
            rc = L.gsim_db_search_labels(main_table._h, ls._h, q.ctypes.data_as(u32p), 5, 30, cutoff, 0, 1.0, 1.0, 0, hits.ctypes.data_as(C.c_void_p),
                                         hit_labels.ctypes.data_as(u32p), counts.ctypes.data_as(u32p), None, None, None, None, None)
            assert rc == 0
            assert np.array_equal(counts, full["counts"])
            for i in range(5):
                assert hits[i, :counts[i]].tobytes() == full["hits"][i, :counts[i]].tobytes()
                assert np.array_equal(hit_labels[i, :counts[i]], full["hit_labels"][i, :counts[i]])
            # one optional output at a time
            approx = np.zeros(5, np.uint64)
            kept = np.zeros((5, nlabels), np.uint32)
            rc = L.gsim_db_search_labels(main_table._h, ls._h, q.ctypes.data_as(u32p), 5, 30, cutoff, 0, 1.0, 1.0, 0, hits.ctypes.data_as(C.c_void_p),
                                         hit_labels.ctypes.data_as(u32p), counts.ctypes.data_as(u32p), approx.ctypes.data_as(u64p), None, None,
                                         kept.ctypes.data_as(u32p), None)
            assert rc == 0 and np.array_equal(approx, full["approx"]) and np.array_equal(kept, full["label_kept"])
        # nq == 0: GSIM_OK, nothing to write
        assert L.gsim_db_search_labels(main_table._h, ls._h, None, 0, 30, 0.0, 0, 1.0, 1.0, 0, hits.ctypes.data_as(C.c_void_p),
                                       hit_labels.ctypes.data_as(u32p), counts.ctypes.data_as(u32p), None, None, None, None, None) == 0


@pytest.mark.parametrize("name", ["uniform 1000", "40000 labels", "cluster order"])
def test_a_row_base_the_launch_cut_and_the_run_change_nothing(name, main_table):
    labels, nlabels = LABELS[N_MAIN][name]
    q = queries(*MAIN)[:5]
    H = pair_hits(*MAIN, "tanimoto", 5)
    for cutoff in (0.0, 0.2):
        w = R.expect(H, labels, nlabels, 40, cutoff)
        with main_table.labelset(labels, nlabels) as ls:
            whole = main_table.search_labels(ls, q, 40, cutoff, per_label=True, stats=True)
            cut = main_table.search_labels(ls, q, 40, cutoff, per_label=True, stats=True, launch_rows=1024)  # twenty launches, the table carried
            again = main_table.search_labels(ls, q, 40, cutoff, per_label=True, stats=True)
        for got in (whole, cut, again):
            R.same(got, w, (name, cutoff))
        for key in ("hits", "hit_labels", "counts", "approx", "rows_kept", "label_best", "label_kept"):
            assert whole[key].tobytes() == again[key].tobytes() == cut[key].tobytes(), key
        assert cut["stats"]["launches"] >= whole["stats"]["launches"] + 19 and again["stats"]["launches"] == whole["stats"]["launches"]
    based = table(data(*MAIN), row_base=1 << 20)
    try:
        with based.labelset(labels, nlabels) as ls:
            R.same(based.search_labels(ls, q, 40, 0.2, per_label=True), R.expect(H, labels, nlabels, 40, 0.2, row_base=1 << 20), (name, "row base"))
    finally:
        based.close()


def test_a_search_before_and_after_returns_the_same_hits(main_table):
    db = data(*MAIN)
    q = db[[17, 1234]]
    before = main_table.search(q, 50, 0.1)
    for name in ("uniform 1000", "40000 labels"):
        labels, nlabels = LABELS[N_MAIN][name]
        with main_table.labelset(labels, nlabels) as ls:
            main_table.search_labels(ls, queries(*MAIN), 10, 0.1, per_label=True)
            main_table.search_labels(ls, q, 10, launch_rows=1024)
    after = main_table.search(q, 50, 0.1)
    assert all(b.tobytes() == a.tobytes() for b, a in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    want_hits, _ = O.search(q[0], db, 50, 0.1, nthreads=4)
    assert len(want_hits) > 0 and np.array_equal(after[0][0]["row"], want_hits["row"])


def test_what_the_call_refuses(main_table):
    L = capi.load()
    labels, nlabels = LABELS[N_MAIN]["uniform 7"]
    q = np.ascontiguousarray(queries(*MAIN)[:2])
    u32p = C.POINTER(C.c_uint32)
    hits = np.zeros((2, 4), capi.HIT_DTYPE)
    hit_labels = np.full((2, 4), 77, np.uint32)
    counts = np.full(2, 77, np.uint32)
    other = table(data(*MAIN))
    wide = capi.Table(4128).add_rows(np.ones((3, 129), np.uint32)).finalize(0, 1)
    host_only = capi.Table(1024).add_rows(np.asarray(data(*MAIN)[:40]))
    ls = main_table.labelset(labels, nlabels)
    theirs = other.labelset(labels, nlabels)
    wide_ls = wide.labelset(np.zeros(3, np.uint32), 1)
    try:
        names = ["db", "ls", "queries", "nq", "k", "cutoff", "metric", "alpha", "beta", "launch_rows", "hits", "hit_labels", "counts", "approx", "rows_kept",
                 "label_best", "label_kept", "stats"]
        ok = [main_table._h, ls._h, q.ctypes.data_as(u32p), 2, 4, 0.0, 0, 1.0, 1.0, 0, hits.ctypes.data_as(C.c_void_p), hit_labels.ctypes.data_as(u32p),
              counts.ctypes.data_as(u32p), None, None, None, None, None]

        def with_(**kw):
            a = list(ok)
            for k, v in kw.items():
                a[names.index(k)] = v
            return tuple(a)
        nan, inf = float("nan"), float("inf")
        cases = {"NULL db": with_(db=None), "NULL ls": with_(ls=None), "NULL hits": with_(hits=None), "NULL hit_labels": with_(hit_labels=None),
                 "NULL counts": with_(counts=None), "NULL queries": with_(queries=None), "another handle's label set": with_(ls=theirs._h),
                 "this label set on another handle": with_(db=other._h), "a label set on a handle without rows on a GPU": with_(db=host_only._h),
                 "an unknown metric": with_(metric=2), "a negative metric": with_(metric=-1), "Tversky alpha < 0": with_(metric=1, alpha=-0.5),
                 "Tversky beta NaN": with_(metric=1, beta=nan), "Tversky alpha infinite": with_(metric=1, alpha=inf),
                 "rows wider than 4096 bits": with_(db=wide._h, ls=wide_ls._h, queries=np.zeros((2, 129), np.uint32).ctypes.data_as(u32p))}
        for what, args in cases.items():
            assert L.gsim_db_search_labels(*args) == -1 and len(L.gsim_last_error()) > 0, what
            assert (counts == 77).all() and (hit_labels == 77).all(), what
        assert b"4096" in L.gsim_last_error()
        assert L.gsim_db_search_labels(*with_(metric=1, alpha=0.0, beta=0.0)) == 0, "Tversky (0, 0) is a valid metric"
        assert L.gsim_db_search_labels(*ok) == 0 and (counts == 4).all()
        out = C.c_void_p(0x1234)
        bad = labels.copy()
        bad[N_MAIN - 1] = nlabels
        assert L.gsim_labelset_create(main_table._h, bad.ctypes.data_as(u32p), nlabels, C.byref(out)) == -1 and not out.value
        folded = capi.Table(1024).add_rows(np.asarray(data(*MAIN)[:4096])).set_fold_factor(2).finalize(0, 1)
        try:
            out = C.c_void_p(0x1234)
            assert L.gsim_labelset_create(folded._h, labels.ctypes.data_as(u32p), nlabels, C.byref(out)) == -5 and not out.value, "a folded table"
        finally:
            folded.close()
    finally:
        for x in (ls, theirs, wide_ls):
            x.close()
        for x in (other, wide, host_only):
            x.close()


def test_a_label_set_serves_many_calls_and_goes(main_table):
    labels, nlabels = LABELS[N_MAIN]["uniform 1000"]
    q = queries(*MAIN)
    H = pair_hits(*MAIN, "tanimoto", NQ)
    w = R.expect(H[:3], labels, nlabels, 5, 0.0)
    ls = main_table.labelset(labels, nlabels)
    for _ in range(25):
        R.same(main_table.search_labels(ls, q[:3], 5), w)
    ls.close()
    ls.close()  # (a second close does nothing)
    with pytest.raises(capi.GsimError) as e:
        main_table.search_labels(ls, q[:3], 5)
    assert e.value.code == -1
    hits, approx = main_table.search(q[:3], 5)
    assert [int(a) for a in approx] == [N_MAIN] * 3
