"""The periodic-table model (tests/periodic_table.py) against the real oracles, on the CPU: the table of 3 P + 17 = 12 314 rows is
MATERIALISED on the host, independently of the model's source map, and every expansion helper -- one per result shape that
tests/test_gpu_large_offsets.py compares -- must give exactly (scores by their bits) what the existing oracle or rule gives on the
materialised rows.  The planting scheme is the GPU test's, scaled down: boundaries at rows 2^11, 2^12, 2^13 and 11 001.

One NEGATIVE CONTROL per shape: the same result computed by the same oracle over the table as a wrapped offset would show it --
every row at or past a boundary b reads row r - 2^m, 2^m the largest power of two not above b -- must DIFFER from the true one, for
every boundary.  That is what makes a passing GPU test mean something: the planted rows and the prime period make a wrap visible in
that call's output."""
import numpy as np
import pytest

import kmeans_rule as R
import oracle_lib as O
import periodic_table as T
from knn_join_rule import knn_join_rule

P = T.P
N = 3 * P + 17
BOUNDARIES = [1 << 11, 1 << 12, 1 << 13, 11001]
SEED = 0x9E1
WIDTHS = [128, 5]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case:
    def __init__(self, W):
        self.W = W
        self.planted, self.info = T.plant(N, W, BOUNDARIES, SEED)
        self.model = T.PeriodicTable(N, W, SEED, self.planted)
        # the table on the host, built without the model's source map
        db = np.tile(O.synth_rows(SEED, O.KIND_SPARSE, 0, P, W), (4, 1))[:N].copy()
        for r, fp in self.planted.items():
            db[r] = fp
        db.setflags(write=False)
        self.db = db
        # the wrapped tables of the negative controls, materialised
        self.controls = []
        for b in BOUNDARIES:
            shift = 1 << (b.bit_length() - 1)
            wdb = db.copy()
            wdb[b:] = db[b - shift:N - shift]
            assert np.array_equal(wdb, self.model.wrapped(b, shift).rows(0, N))
            self.controls.append(wdb)


_cases = {}


@pytest.fixture(params=WIDTHS, ids=lambda W: "%dbits" % (W * 32))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def S_of(left, db, kw):
    return R.score_matrix(np.ascontiguousarray(left, dtype=np.uint32), db, kw)


def test_the_block_rows_are_distinct_and_the_rows_are_the_materialised_ones(case):
    m, db = case.model, case.db
    assert len(np.unique(m.block, axis=0)) == P
    assert np.array_equal(m.rows(0, N), db) and np.array_equal(m.row(N - 1), db[N - 1])
    assert np.array_equal(m.rows(4000, 4200), db[4000:4200])
    rows = np.array([0, 5, 2047, 2048, 2049, P, P + 1, N - 21, N - 1])
    assert np.array_equal(m.take_rows(rows), db[rows])
    info = case.info
    assert not db[info["zero"]].any() and all((db[r] == 0xFFFFFFFF).all() for r in info["ones"])
    assert len(info["family"]) >= 20 and len(np.unique(info["family"], axis=0)) == len(info["family"])
    for b in BOUNDARIES:  # a run of variants straddles every boundary
        assert b - 1 in info["variant_row"] and b in info["variant_row"]
    T.past(info["variant_row"], info)


def test_multiplicity_and_replicas_against_the_materialised_source_map(case):
    m = case.model
    src = m.source_of(np.arange(N))
    assert np.array_equal(case.db, m.sources()[src])
    want = np.bincount(src, minlength=m.U)
    assert np.array_equal(m.multiplicities(), want) and np.array_equal(m.multiplicities(generic=True), want) and want.sum() == N
    for u in list(range(0, P, 37)) + [2047 % P, 2048 % P, 11001 % P] + list(range(P, m.U)):
        where = np.flatnonzero(src == u)
        assert m.multiplicity(u) == len(where) == m.multiplicity(u, generic=True)
        assert np.array_equal(m.replicas(u), where) and np.array_equal(m.replicas(u, generic=True), where)
        for limit in (1, 2, 3, 128):
            assert np.array_equal(m.replicas(u, limit), where[:limit])


def test_column_counts(case):
    m, db = case.model, case.db
    want = T.unpack(db).sum(axis=0, dtype=np.uint64)
    counts, counted = m.expand_counts()
    assert counted == N and counts.dtype == np.uint64 and np.array_equal(counts, want)
    for wdb in case.controls:
        assert not np.array_equal(T.unpack(wdb).sum(axis=0, dtype=np.uint64), want), "control"


def test_row_vectors_overlap_sums_and_assignment(case):
    m, db, info = case.model, case.db, case.info
    weights = np.random.default_rng(3).integers(0, 2**32, m.W * 32, dtype=np.uint64)
    want = T.unpack(db).astype(np.uint64) @ weights
    per_source = T.unpack(m.sources()).astype(np.uint64) @ weights
    assert np.array_equal(m.expand_vector(per_source), want)
    assert np.array_equal(m.expand_vector(per_source, 4000, 4200), want[4000:4200])
    for wdb in case.controls:
        assert not np.array_equal(T.unpack(wdb).astype(np.uint64) @ weights, want), "control"
    C = T.centres(m, info)
    for kw in T.METRICS:
        label, score = R.assign(S_of(C, db, kw))
        lu, su = R.assign(T.score_matrix(C, m, kw))
        assert np.array_equal(m.expand_vector(lu), label) and np.array_equal(bits(m.expand_vector(su)), bits(score))
        assert (label[info["variant_row"]] == len(C) - 1).all(), "the family's rows are assigned to F"
        for wdb in case.controls:
            wl, ws = R.assign(S_of(C, wdb, kw))
            assert not np.array_equal(wl, label) and not np.array_equal(bits(ws), bits(score)), "control"


def test_the_tiled_route_of_expand_vector():
    """whole large tables take np.tile instead of a source map of every row: the same vector"""
    n, W = (1 << 22) + 5 * P + 3, 5
    planted, info = T.plant(n, W, [1 << 20, 1 << 22], SEED)
    m = T.PeriodicTable(n, W, SEED, planted)
    per_source = np.random.default_rng(1).integers(0, 2**32, m.U, dtype=np.uint64)
    want = np.take(per_source, m.source_of(np.arange(n)))
    assert np.array_equal(m.expand_vector(per_source), want)
    lo = (1 << 20) - 77
    assert np.array_equal(m.expand_vector(per_source, lo, n - 1), want[lo:n - 1])


def test_label_counts(case):
    m, db = case.model, case.db
    planted_labels = np.array([7 + i % 2 if i % 5 else R.LABEL_NONE for i in range(len(m.prow))], np.uint32)
    labels = m.labels(7, planted_labels)
    assert np.array_equal(np.delete(labels, m.prow), np.delete(np.arange(N) % 7, m.prow)) and (labels[m.prow] == planted_labels).all()
    want = R.label_counts(db, labels, 9)
    got = m.expand_label_counts(7, 9, planted_labels)
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[1][7] > 0 and want[1][8] > 0 and want[1].sum() == N - (planted_labels == R.LABEL_NONE).sum()
    lo, hi = 4000, 4200
    assert np.array_equal(m.labels(7, planted_labels, lo, hi), labels[lo:hi])
    for wdb in case.controls:
        assert not np.array_equal(R.label_counts(wdb, labels, 9)[0], want[0]), "control"


def oracle_join(left, db, cutoff, kw):
    """what tests/test_gpu_join.py expects: list i = the oracle's search(left[i], k = N, cutoff), by row"""
    indptr, ind, sc = [0], [], []
    for q in left:
        hits, approx = O.search(q, db, len(db), cutoff, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        assert len(hits) == approx
        hits = hits[np.argsort(hits["row"], kind="stable")]
        ind.append(hits["row"].astype(np.uint32))
        sc.append(hits["score"])
        indptr.append(indptr[-1] + len(hits))
    return np.array(indptr, np.uint64), np.concatenate(ind), np.concatenate(sc)


def test_threshold_lists(case):
    m, db, info = case.model, case.db, case.info
    fam, blk = T.family_left(info), np.ascontiguousarray(m.block[[5, 2048 % P, 4000]])
    for kw in T.METRICS:
        S = T.score_matrix(fam, m, kw)
        cutoff = T.family_cutoff(S, m, info)
        want = oracle_join(fam, db, cutoff, kw)
        assert same_csr(m.expand_csr(S, cutoff), want)
        assert all(set(want[1][want[0][i]:want[0][i + 1]].tolist()) >= set(info["variant_row"].tolist()) for i in range(len(fam)))
        T.past(want[1], info)
        for wdb in case.controls:
            assert not same_csr(oracle_join(fam, wdb, cutoff, kw), want), "control"
        # copies of block rows at cutoff 1.0: each list is the row's replicas
        S1 = T.score_matrix(blk, m, kw)
        want = oracle_join(blk, db, 1.0, kw)
        assert same_csr(m.expand_csr(S1, 1.0), want)
        assert np.array_equal(want[1][:int(want[0][1])], m.replicas(5)) and m.multiplicity(5) == 3, "(3 P + 5 is a planted row)"
        assert int(want[1][-1]) == 2 * P + 4000 >= BOUNDARIES[-1]
        for wdb in case.controls:
            assert not same_csr(oracle_join(blk, wdb, 1.0, kw), want), "control"


def test_knn_lists(case):
    m, db, info = case.model, case.db, case.info
    fam, blk = T.family_left(info), np.ascontiguousarray(m.block[[5, 4000]])
    for kw in T.METRICS:
        S, Sdb = T.score_matrix(fam, m, kw), S_of(fam, db, kw)
        cutoff = T.family_cutoff(S, m, info)
        for k in (1, 5, 128):
            want = knn_join_rule(Sdb, k, cutoff)
            assert same_csr(m.expand_csr(S, cutoff, k), want)
            for wdb in case.controls:  # (k = 1 lists hold three rows in all: not every boundary's wrap moves one of them)
                assert k == 1 or not same_csr(knn_join_rule(S_of(fam, wdb, kw), k, cutoff), want), "control"
        S1, S1db = T.score_matrix(blk, m, kw), S_of(blk, db, kw)
        for k in (1, 5, 128):
            want = knn_join_rule(S1db, k, T.TINY)
            assert same_csr(m.expand_csr(S1, T.TINY, k), want)
        assert np.array_equal(want[1][:3], m.replicas(5)) and (want[2][:3] == 1.0).all(), "the tie rule: the replicas first, by row"
        for wdb in case.controls:
            assert not same_csr(knn_join_rule(S_of(blk, wdb, kw), 128, T.TINY), want), "control"


def oracle_knn(db, owners, k, cutoff, kw):
    """gsim_db_knn's rule as the header states it: search(row i, k + 1, cutoff) minus row i, cut to k"""
    indptr, ind, sc = [0], [], []
    for i in owners:
        hits, _ = O.search(db[i], db, (len(db) if k is None else k + 1), cutoff, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        hits = hits[hits["row"] != i][:k]
        if k is None:  # gsim_db_neighbors: every row at or above the cutoff but row i, by column
            hits = hits[np.argsort(hits["row"], kind="stable")]
        ind.append(hits["row"].astype(np.uint32))
        sc.append(hits["score"])
        indptr.append(indptr[-1] + len(hits))
    return np.array(indptr, np.uint64), np.concatenate(ind), np.concatenate(sc)


def test_knn_and_neighbour_lists_of_a_row_range(case):
    m, db, info = case.model, case.db, case.info
    lo, hi = info["tail"]
    owners = np.arange(lo, hi)
    for kw in T.METRICS:
        S = T.score_matrix(m.rows(lo, hi), m, kw)
        cutoff = T.family_cutoff(S, m, info)
        for k in (1, 5, 128, None):
            want = oracle_knn(db, owners, k, cutoff, kw)
            assert same_csr(m.expand_csr(S, cutoff, k, self_rows=owners), want), (kw, k)
            if k in (128, None):
                T.past(want[1], info)
                for wdb in case.controls[:-1]:  # (the last boundary's wrap moves the owners themselves: the range reads other rows)
                    assert not same_csr(oracle_knn(wdb, owners, k, cutoff, kw), want), "control"
        assert not np.array_equal(db[lo:hi], case.controls[-1][lo:hi])
        # neighbour lists at 1.0 of owners that are block rows: their replicas
        own1 = np.arange(BOUNDARIES[-1] + 100, BOUNDARIES[-1] + 164)
        assert not np.isin(own1, m.prow).any()
        S1 = T.score_matrix(db[own1], m, kw)
        want = oracle_knn(db, own1, None, 1.0, kw)
        assert same_csr(m.expand_csr(S1, 1.0, None, self_rows=own1), want)
        assert (np.diff(want[0].astype(np.int64)) >= 2).all()
        for wdb in case.controls[:-1]:
            assert not same_csr(oracle_knn(wdb, own1, None, 1.0, kw), want), "control"


def test_histograms(case):
    m, db, info = case.model, case.db, case.info
    left = T.mixed_left(m, info)
    for kw in T.METRICS:
        S, Sdb = T.score_matrix(left, m, kw), S_of(left, db, kw)
        edges = T.data_edges(S)
        nb = len(edges) + 1
        want = np.stack([np.bincount(b, minlength=nb) for b in T.hist_bins(Sdb, edges)]).astype(np.uint64)
        assert np.array_equal(m.expand_hist(T.hist_bins(S, edges), nb), want) and (want.sum(axis=1) == N).all()
        assert (want > 0).sum(axis=0).min() > 0, "every bin is used"
        for wdb in case.controls:
            w = np.stack([np.bincount(b, minlength=nb) for b in T.hist_bins(S_of(left, wdb, kw), edges)]).astype(np.uint64)
            assert not np.array_equal(w, want), "control"
        # the table against a range of itself, the pair (row i, row i) not counted
        lo, hi = BOUNDARIES[-1] - 10, BOUNDARIES[-1] + 60
        own = np.arange(lo, hi)
        Sown, Sown_db = T.score_matrix(db[lo:hi], m, kw), S_of(db[lo:hi], db, kw)
        bins = T.hist_bins(Sown_db, edges)
        want = np.stack([np.bincount(b, minlength=nb) for b in bins]).astype(np.uint64)
        want[np.arange(hi - lo), bins[np.arange(hi - lo), own]] -= 1
        assert np.array_equal(m.expand_hist(T.hist_bins(Sown, edges), nb, self_rows=own), want)


def test_score_matrices(case):
    m, db, info = case.model, case.db, case.info
    left = T.mixed_left(m, info)
    for kw in T.METRICS:
        S, Sdb = T.score_matrix(left, m, kw), S_of(left, db, kw)
        assert np.array_equal(bits(m.expand_vector(S.T).T), bits(Sdb))
        for (lo, hi), wdb in zip(T.straddles(m, info, 1000), case.controls):
            cols = np.arange(lo, hi)
            assert np.array_equal(bits(S[:, m.source_of(cols)]), bits(Sdb[:, lo:hi]))
            assert not np.array_equal(bits(S_of(left, wdb[lo:hi], kw)), bits(Sdb[:, lo:hi])), "control"


def group_expected(g, which, cutoff, k, model, popc):
    """a group query's hits from the per-source group scores, through expand_csr"""
    csr = model.expand_csr(g[None, :], cutoff, k)
    src = model.source_of(csr[1])
    return csr[1], csr[2], which[src], popc[src], int(model.multiplicities()[g >= F(cutoff)].sum())


def test_group_queries(case):
    m, db, info = case.model, case.db, case.info
    queries = np.ascontiguousarray(info["family"][[0, 2, 4, 9, 13]])
    popc_db = T.unpack(db).sum(axis=1)
    for kw in T.METRICS:
        S, Sdb = T.score_matrix(queries, m, kw), S_of(queries, db, kw)
        for mode in ("max", "mean"):
            g, which = (S.max(0), S.argmax(0)) if mode == "max" else (T.mean_in_order(S), np.zeros(m.U, np.int64))
            gdb, whichdb = (Sdb.max(0), Sdb.argmax(0)) if mode == "max" else (T.mean_in_order(Sdb), np.zeros(N, np.int64))
            cutoff = T.cutoff_between(g[:P], g[T.family_sources(m, info)])
            rows, s, approx = O.canonical_topk_from_scores(gdb, 100, cutoff)
            got = group_expected(g, which, cutoff, 100, m, T.unpack(m.sources()).sum(axis=1))
            assert np.array_equal(got[0], rows) and np.array_equal(bits(got[1]), bits(s)) and got[4] == approx
            assert np.array_equal(got[2], whichdb[rows]) and np.array_equal(got[3], popc_db[rows])
            T.past(rows, info)
            for wdb in case.controls:
                Sw = S_of(queries, wdb, kw)
                gw = Sw.max(0) if mode == "max" else T.mean_in_order(Sw)
                wr, ws, _ = O.canonical_topk_from_scores(gw, 100, cutoff)
                assert not (np.array_equal(wr, rows) and np.array_equal(bits(ws), bits(s))), "control"


def test_row_set_searches_and_counts(case):
    """gsim_db_search_rows and gsim_db_bit_counts(rowset) take their expected values from the set's own host rows (model.take_rows):
    those must be the materialised rows, the set must hold the planted rows and both sides of every boundary, and a wrap must show."""
    m, db, info = case.model, case.db, case.info
    rows = T.boundary_rowset(m, info, 300)
    assert np.isin(m.prow, rows).all() and all(b - 300 in rows and b + 299 in rows for b in BOUNDARIES) and N - 1 in rows
    sub = m.take_rows(rows)
    assert np.array_equal(sub, db[rows])
    want_counts = T.unpack(sub).sum(axis=0, dtype=np.uint64)
    for kw in T.METRICS:
        q = info["family"][0]
        hits, approx = O.search(q, sub, 100, 0.0, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        T.past(rows[hits["row"]], info)
        for wdb in case.controls:
            wh, _ = O.search(q, wdb[rows], 100, 0.0, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0))
            assert not (np.array_equal(wh["row"], hits["row"]) and np.array_equal(bits(wh["score"]), bits(hits["score"]))), "control"
    for wdb in case.controls:
        assert not np.array_equal(T.unpack(wdb[rows]).sum(axis=0, dtype=np.uint64), want_counts), "control"
