"""The analytic calls on tables past the 2 GiB, 4 GiB and 16 GiB offsets: every call that streams a whole table against a few rows,
on tables large enough that a byte offset, a word index or a row number computed in 32 bits would wrap -- compared exactly
(indices, counts, scores by their bits) with the periodic-table model of tests/periodic_table.py, whose helpers
tests/test_periodic_model_host.py checks against the real oracles on the CPU, each with a negative control.

shape      rows                                   size                 what it crosses
small      3 P + 17 = 12 314, 4096 and 160 bits   under 7 MB           nothing: the same assertions, so that a mistake of this file
                                                                       shows here first
A          2^25 + 2^21 + 3 x 4096 bits (W = 128)  17.0 GiB             byte offset 2^31 (row 2^22) and 2^32 (row 2^23), word index
                                                                       2^31 (row 2^24) and 2^32 (row 2^25)
B          216 000 003 x 160 bits (W = 5, the     4.0 GiB, 6.4 GiB     byte offset 2^31 and 2^32 in the raw rows (rows 107 374 183,
           tile kernels' padded copy WP = 8)      padded               214 748 365) and in the padded copy (rows 2^26, 2^27); row
                                                                       numbers above 2^27

NOT covered: the u32x4-unit index reaches 2^32 only at 64 GiB and a raw word index at 160 bits only past 859 M rows; the all-pairs-only
calls (components, mst, leader, kmeans -- kmeans only through assign and label_counts).

Device memory: shape B asks for 14 GiB -- the 4.0 GiB table and ONE padded copy of 6.4 GiB.  A padded copy belongs to a call, not to
a handle (the calls' PaddedRows are locals, freed on return), so the second handle that the route tests attach adds none.

The tables are built by torch, not by the library: the 4099-row block repeated, the planted rows written with index_copy_, the tensor
handed over with gsim_db_attach_device_rows -- the content owes nothing to the code under test.  Every expected value comes from
oracle_lib, a *_rule.py or numpy, through the model.  One shape is alive at a time (a module-scoped fixture; the tests are grouped
by its parameter).  Every test first asserts on the EXPECTED result that it is not vacuous: at least 20 expected rows at or past the
last boundary and one past each (periodic_table.past), or the like for results that are not lists."""
import contextlib
import os

import numpy as np
import pytest

import kmeans_rule as R
import oracle_lib as O
import periodic_table as T
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
P = T.P
GIB = 1 << 30
SEED = 0x9E1
F = np.float32

SHAPES = {
    #            rows                         W    boundaries                                              free HBM needed
    "small4096": (3 * P + 17,                 128, [1 << 11, 1 << 12, 1 << 13, 11001],                     0),
    "small160":  (3 * P + 17,                 5,   [1 << 11, 1 << 12, 1 << 13, 11001],                     0),
    "A":         ((1 << 25) + (1 << 21) + 3,  128, [1 << 22, 1 << 23, 1 << 24, 1 << 25],                   24 * GIB),
    "B":         (216_000_003,                5,   [1 << 26, 107_374_183, 1 << 27, 214_748_365],           14 * GIB),
}
ALL = ["small4096", "small160", "A", "B"]
NOT_B = ALL[:3]  # (a prefix of ALL: the module-scoped fixture sees the same parameter index for the same shape)
# The default launch plans are cut by size nowhere else in the suite: on shape A these calls must have made more than one launch
# (the others' plans do not cut at 17 GiB, or have one launch by design: their counts are printed only).
CUT_ON_A = {"assign", "join, tiles", "knn_join", "knn", "neighbors", "histogram, tiles", "search_group"}


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


class Shape:
    def __init__(self, name):
        import torch
        self.name = name
        self.n, self.W, boundaries, need = SHAPES[name]
        self.big = need > 0
        if self.big:
            free = capi.device_free_bytes(0)
            if free < need:
                pytest.skip("needs %.0f GiB of free HBM, %.0f GiB free" % (need / GIB, free / GIB))
        # row offsets are what the shapes are about: check the arithmetic of the table above
        if name == "A":
            assert [b * 512 for b in boundaries[:2]] == [1 << 31, 1 << 32] and [b * 128 for b in boundaries[2:]] == [1 << 31, 1 << 32]
        if name == "B":
            assert [boundaries[0] * 32, boundaries[2] * 32] == [1 << 31, 1 << 32]
            assert all((b - 1) * 20 < lim <= b * 20 for b, lim in ((boundaries[1], 1 << 31), (boundaries[3], 1 << 32)))
        planted, self.info = T.plant(self.n, self.W, boundaries, SEED)
        self.model = m = T.PeriodicTable(self.n, self.W, SEED, planted)
        block = torch.from_numpy(m.block.view(np.int32)).cuda()
        self.ten = block.repeat((self.n + P - 1) // P, 1)[:self.n]
        self.ten.index_copy_(0, torch.from_numpy(m.prow).cuda(), torch.from_numpy(m.pfp.view(np.int32)).cuda())
        torch.cuda.synchronize()
        assert self.ten.dtype == torch.int32 and tuple(self.ten.shape) == (self.n, self.W) and self.ten.is_contiguous()
        self.table = self.attach()
        assert self.table.count() == self.n
        from conftest import record_parity
        record_parity("large offsets, shape %s" % name, "periodic model", "%d rows x %d bits, %.1f GiB" % (self.n, self.W * 32, self.n * self.W * 4 / GIB))

    def attach(self, **kn):
        """another handle on the same rows, created under the given knobs"""
        with knobs(**kn):
            return capi.Table(self.W * 32).attach_device_rows(self.ten.data_ptr(), self.n, 0)

    def left_table(self, rows):
        return capi.Table(self.W * 32).add_rows(np.ascontiguousarray(rows, dtype=np.uint32)).finalize(0, 1)

    def launches(self, call, count):
        """the default plan's launches: printed on every shape, asserted on shape A for the calls of CUT_ON_A"""
        print("%s: %s made %d launches" % (self.name, call, count))
        assert self.name != "A" or call not in CUT_ON_A or count > 1, (call, count)

    def close(self):
        import torch
        self.table.close()
        del self.ten
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def shape(request):
    sh = Shape(request.param)
    yield sh
    sh.close()


def every(shapes):
    return pytest.mark.parametrize("shape", shapes, indirect=True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_csr(got, want, what):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (what, "indptr")
    assert np.array_equal(got[1], want[1]), (what, "indices")
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, "scores")


def counts_of(rows):
    return T.unpack(rows).sum(axis=0, dtype=np.uint64)


def kwargs(kw):
    return dict(metric=kw.get("metric", 0), alpha=kw.get("alpha", 1.0), beta=kw.get("beta", 1.0))


@every(ALL)
def test_the_table_is_the_models(shape):
    """rows read back through the library (one hipMemcpy each, no kernel) on both sides of every boundary"""
    m, info = shape.model, shape.info
    for r in [0, P, info["zero"], shape.n - 1] + [b + d for b in info["boundaries"] for d in (-2, -1, 0, 1, 2)]:
        assert np.array_equal(shape.table.row(r), m.row(r)), r


@every(NOT_B)
def test_bit_counts_and_overlap_sums(shape):
    m, info, t = shape.model, shape.info, shape.table
    want, _ = m.expand_counts()
    plain = (np.ceil(shape.n / P) * counts_of(m.block)).astype(np.uint64)
    assert not np.array_equal(want, plain) and want.min() > 0, "the planted rows and the cut period show in the expected counts"
    st = {}
    counts, counted = t.bit_counts(stats=st)
    shape.launches("bit_counts", st["launches"])
    assert counted == shape.n and np.array_equal(counts, want)
    ranges = T.straddles(m, info, 10000 if shape.big else 1000)
    for lo, hi in ranges:
        counts, counted = t.bit_counts(row_begin=lo, row_end=hi)
        assert counted == hi - lo and np.array_equal(counts, counts_of(m.rows(lo, hi))), (lo, hi)
    weights = np.random.default_rng(shape.W).integers(0, 2**32, shape.W * 32, dtype=np.uint64)
    B = T.unpack(m.sources())
    per_source, popc = B.astype(np.uint64) @ weights, B.sum(axis=1, dtype=np.uint32)
    assert len(np.unique(per_source)) == len(np.unique(m.sources(), axis=0)), "every source row has a sum of its own: a misread row shows"
    st = {}
    sums, pc = t.overlap_sums(weights, popc=True, stats=st)
    shape.launches("overlap_sums", st["launches"])
    assert np.array_equal(sums, m.expand_vector(per_source)) and np.array_equal(pc, m.expand_vector(popc))
    assert all(int(pc[r]) == shape.W * 32 for r in info["ones"]) and int(pc[info["zero"]]) == 0
    for lo, hi in ranges:
        sums, pc = t.overlap_sums(weights, lo, hi, popc=True)
        assert np.array_equal(sums, m.expand_vector(per_source, lo, hi)) and np.array_equal(pc, m.expand_vector(popc, lo, hi)), (lo, hi)


@every(NOT_B)
def test_label_counts(shape):
    m, info, t = shape.model, shape.info, shape.table
    planted_labels = np.array([7 + i % 2 if i % 5 else capi.LABEL_NONE for i in range(len(m.prow))], np.uint32)
    want = m.expand_label_counts(7, 9, planted_labels)
    assert want[1][7] > 0 and want[1][8] > 0 and int(want[1].astype(np.int64).sum()) == shape.n - int((planted_labels == capi.LABEL_NONE).sum())
    labels = m.labels(7, planted_labels)
    st = {}
    counts, sizes = t.label_counts(labels, 9, stats=st)
    shape.launches("label_counts", st["launches"])
    assert np.array_equal(sizes, want[1]) and np.array_equal(counts, want[0])
    for lo, hi in T.straddles(m, info, 10000 if shape.big else 1000):
        counts, sizes = t.label_counts(labels[lo:hi], 9, row_begin=lo, row_end=hi)
        w = R.label_counts(m.rows(lo, hi), labels[lo:hi], 9)
        assert w[1][7] + w[1][8] > 0 and np.array_equal(sizes, w[1]) and np.array_equal(counts, w[0]), (lo, hi)


def the_row_set(shape):
    """the planted rows and a few thousand rows on either side of every boundary, and the table's last rows"""
    m, info = shape.model, shape.info
    rows = T.boundary_rowset(m, info, 3000 if shape.big else 300)
    assert np.isin(m.prow, rows).all()
    T.past(rows, info)
    bitmap = np.zeros((shape.n + 31) // 32, np.uint32)
    np.bitwise_or.at(bitmap, rows // 32, (np.uint32(1) << (rows % 32).astype(np.uint32)))
    return rows, bitmap, m.take_rows(rows)


@every(NOT_B)
@pytest.mark.parametrize("route", ["0", "1000"], ids=["stream", "gather"])
def test_bit_counts_of_a_row_set(shape, route):
    rows, bitmap, sub = the_row_set(shape)
    want = counts_of(sub)
    t = shape.attach(GSIM_SUBSET_GATHER_MAX_PERMILLE=route)
    try:
        for what, rs in (("rows", t.rowset(rows=rows.astype(np.uint32))), ("bitmap", t.rowset(bitmap=bitmap))):
            st = {}
            counts, counted = t.bit_counts(rs, stats=st)
            assert counted == len(rows) and np.array_equal(counts, want), what
            assert st["route"] == (capi.PROFILE_GATHERED if route == "1000" else capi.PROFILE_STREAMED)
            assert st["rows_read"] == (len(rows) if route == "1000" else shape.n)
            # the set cut by a range that begins past the last boundary
            lo = shape.info["boundaries"][-1] - 5
            inside = rows >= lo
            counts, counted = t.bit_counts(rs, row_begin=lo, row_end=shape.n)
            assert counted == int(inside.sum()) and np.array_equal(counts, counts_of(sub[inside])), what
            rs.close()
    finally:
        t.close()


@every(NOT_B)
@pytest.mark.parametrize("route", ["0", "1000"], ids=["stream", "gather"])
def test_search_rows(shape, route):
    m, info = shape.model, shape.info
    rows, bitmap, sub = the_row_set(shape)
    queries = np.ascontiguousarray(np.stack([info["family"][0], info["family"][6], m.block[info["boundaries"][-1] % P]]))
    t = shape.attach(GSIM_SUBSET_GATHER_MAX_PERMILLE=route)
    try:
        rs = t.rowset(rows=rows.astype(np.uint32))
        assert rs.count == len(rows)
        for kw in T.METRICS:
            hits, approx, st = t.search_rows(rs, queries, 100, 0.0, stats=True, **kwargs(kw))
            assert st["queries_gather"] == (len(queries) if route == "1000" else 0) and st["queries_stream"] == (len(queries) if route == "0" else 0)
            shape.launches("search_rows, " + route, st["launches"])
            for i, q in enumerate(queries):
                want, wap = O.search(q, sub, 100, 0.0, nthreads=16, **kwargs(kw))
                want["row"] = rows[want["row"]]
                if i < 2:
                    T.past(want["row"], info)
                assert len(want) == 100 and int(approx[i]) == wap
                assert np.array_equal(hits[i]["row"], want["row"]) and np.array_equal(bits(hits[i]["score"]), bits(want["score"])), (kw, i)
                assert np.array_equal(hits[i]["common"], want["common"]) and np.array_equal(hits[i]["popc_db"], want["popc_db"]), (kw, i)
        rs.close()
    finally:
        t.close()


@every(ALL)
@pytest.mark.parametrize("kw", T.METRICS, ids=["tanimoto", "tversky"])
def test_assign(shape, kw):
    """130 centres (two centre blocks): the label and the score of all n rows, then of ranges that straddle every boundary"""
    m, info, t = shape.model, shape.info, shape.table
    C = T.centres(m, info)
    lu, su = R.assign(T.score_matrix(C, m, kw))
    assert (lu[T.family_sources(m, info)] == len(C) - 1).all() and len(np.unique(lu)) > 100, "the family goes to F, the last centre"
    want_l, want_s = m.expand_vector(lu), m.expand_vector(su)
    T.past(np.flatnonzero(want_l[info["boundaries"][0]:] == len(C) - 1) + info["boundaries"][0], info)
    st = {}
    label, score = t.assign(C, stats=st, **kwargs(kw))
    shape.launches("assign", st["launches"])
    assert np.array_equal(label, want_l) and np.array_equal(bits(score), bits(want_s))
    del label, score, want_l, want_s
    for lo, hi in T.straddles(m, info, 10000 if shape.big else 1000):
        label, score = t.assign(C, lo, hi, **kwargs(kw))
        assert np.array_equal(label, m.expand_vector(lu, lo, hi)) and np.array_equal(bits(score), bits(m.expand_vector(su, lo, hi))), (lo, hi)


def planted_lists(shape, left, cutoff, kw):
    """Threshold lists at the family's cutoff hold planted rows only (asserted by family_cutoff: no block row reaches it): the oracle's
    search over the planted rows alone, their indices mapped back to the table's."""
    m = shape.model
    indptr, ind, sc = [0], [], []
    for q in left:
        hits, _ = O.search(q, m.pfp, len(m.pfp), cutoff, **kwargs(kw))
        hits = hits[np.argsort(hits["row"], kind="stable")]  # (the planted rows are held ascending by row)
        ind.append(m.prow[hits["row"]].astype(np.uint32))
        sc.append(hits["score"])
        indptr.append(indptr[-1] + len(hits))
    return np.array(indptr, np.uint64), np.concatenate(ind), np.concatenate(sc)


@every(ALL)
@pytest.mark.parametrize("route", ["2147483647", "0"], ids=["stream", "tiles"])
def test_join(shape, route):
    m, info = shape.model, shape.info
    fam = T.family_left(info)
    blk = np.ascontiguousarray(m.block[[5, info["boundaries"][-1] % P, (shape.n - 30) % P, 4000]])
    t = shape.attach(GSIM_JOIN_STREAM_MAX_ROWS=route)
    lfam, lblk = shape.left_table(fam), shape.left_table(blk)
    try:
        for kw in T.METRICS:
            S = T.score_matrix(fam, m, kw)
            cutoff = T.family_cutoff(S, m, info)
            want = planted_lists(shape, fam, cutoff, kw)
            T.past(want[1], info)
            assert all(np.isin(info["variant_row"], want[1][int(a):int(b)]).all() for a, b in zip(want[0][:-1], want[0][1:]))
            st = {}
            same_csr(t.join(fam, cutoff, stats=st, **kwargs(kw)), want, (kw, "family, host queries"))
            assert st["rows_streamed"] == (len(fam) if route != "0" else 0) and st["rows_tiled"] == (len(fam) if route == "0" else 0)
            shape.launches("join, " + ("tiles" if route == "0" else "stream"), st["tile_launches"] + st["stream_launches"])
            same_csr(t.join(lfam, cutoff, **kwargs(kw)), want, (kw, "family, a handle"))
            # copies of block rows at 1.0: each list is that row's replicas, up to the table's last rows
            S1 = T.score_matrix(blk, m, kw)
            want = m.expand_csr(S1, 1.0)
            if shape.big:
                T.past(want[1], info)
            assert np.array_equal(want[1][:int(want[0][1])], m.replicas(5)) and (np.diff(want[0].astype(np.int64)) >= shape.n // P - 1).all()
            assert int(want[1].max()) >= max(shape.n - P, info["boundaries"][-1]), "the lists reach the table's last rows"
            same_csr(t.join(blk, 1.0, **kwargs(kw)), want, (kw, "replicas, host queries"))
            same_csr(t.join(lblk, 1.0, **kwargs(kw)), want, (kw, "replicas, a handle"))
    finally:
        for x in (lfam, lblk, t):
            x.close()


@every(ALL)
@pytest.mark.parametrize("kw", T.METRICS, ids=["tanimoto", "tversky"])
def test_knn_join(shape, kw):
    """GSIM_KNN_JOIN_SEGMENTS unset: the default plan cuts the table into column segments and merges them in one launch.
    gsim_db_knn_queries (host rows) and gsim_db_knn_join (a handle) at every k."""
    m, info, t = shape.model, shape.info, shape.table
    assert "GSIM_KNN_JOIN_SEGMENTS" not in os.environ
    fam = T.family_left(info)
    blk = np.ascontiguousarray(m.block[[5, (shape.n - 30) % P]])
    lfam, lblk = shape.left_table(fam), shape.left_table(blk)
    try:
        S, S1 = T.score_matrix(fam, m, kw), T.score_matrix(blk, m, kw)
        cutoff = T.family_cutoff(S, m, info)
        for k in (1, 5, 128):
            want = m.expand_csr(S, cutoff, k)
            lens = np.diff(want[0].astype(np.int64))
            assert (lens == k).all() if k < 128 else (lens >= len(info["family"])).all(), "k = 1, 5: the lists cut inside the family"
            if k == 128:
                T.past(want[1], info)
            st = {}
            same_csr(t.knn_join(fam, k, cutoff, stats=st, **kwargs(kw)), want, (kw, k, "family, host queries"))
            assert st["segments"] > 1 and st["merge_launches"] == 1, st
            shape.launches("knn_join", st["fold_launches"])
            same_csr(t.knn_join(lfam, k, cutoff, **kwargs(kw)), want, (kw, k, "family, a handle"))
            # a block row at TINY: its replicas tie at 1.0 and the lowest rows are kept
            want = m.expand_csr(S1, T.TINY, k)
            nrep = min(k, m.multiplicity(5))
            assert np.array_equal(want[1][:nrep], m.replicas(5, k)) and (want[2][:nrep] == 1.0).all() and (not shape.big or nrep == k)
            same_csr(t.knn_join(blk, k, T.TINY, **kwargs(kw)), want, (kw, k, "replicas, host queries"))
            same_csr(t.knn_join(lblk, k, T.TINY, **kwargs(kw)), want, (kw, k, "replicas, a handle"))
    finally:
        lfam.close()
        lblk.close()


def tail_owners(shape, kw):
    """the owners of the row-range tests: the family's run in the table's last rows, past every boundary -- their neighbours are the
    other variants, in every run.  -> (lo, hi, owners, S over the sources, the family's cutoff)"""
    m, info = shape.model, shape.info
    lo, hi = info["tail"]
    assert lo > info["boundaries"][-1]
    S = T.score_matrix(m.rows(lo, hi), m, kw)
    return lo, hi, np.arange(lo, hi), S, T.family_cutoff(S, m, info)


@every(ALL)
def test_knn_of_a_row_range(shape):
    """gsim_db_knn over the 20 owners of the table's last rows.  The call spreads owner rows 256 to a workgroup and every workgroup
    walks all N candidate rows itself (include/gpusim_hip.h, gsim_db_knn, "Execution"): the smallest owner range costs what 256
    owners cost, about two minutes on shape A and over one on shape B (the default plan: 3 979 and 10 417 launches).  So the large
    shapes make ONE call, k = 128 under Tversky; the small shapes every k and both metrics.  The faster route the header names for
    such a range, gsim_db_knn_join with left == db and GSIM_KNN_EXCLUDE_SELF, promises the same bytes: compared at every k, both
    metrics, on every shape."""
    m, info, t = shape.model, shape.info, shape.table
    for kw in T.METRICS:
        lo, hi, owners, S, cutoff = tail_owners(shape, kw)
        for k in (1, 5, 128):
            want = m.expand_csr(S, cutoff, k, self_rows=owners)
            if k == 128:
                T.past(want[1], info)
                assert (np.diff(want[0].astype(np.int64)) >= len(info["family"]) - 1).all()
            same_csr(t.knn_join(t, k, cutoff, row_begin=lo, row_end=hi, exclude_self=True, **kwargs(kw)), want, (kw, k, "knn_join, exclude_self"))
            if not shape.big or (k == 128 and kw is T.TV):
                st = {}
                same_csr(t.knn(k, cutoff, row_begin=lo, row_end=hi, stats=st, **kwargs(kw)), want, (kw, k, "knn"))
                shape.launches("knn", st["launches"])


@every(ALL)
def test_neighbors_of_a_row_range(shape):
    """the owners are the family's run in the table's last rows; then 64 owners that are block rows, at 1.0: their replicas"""
    m, info, t = shape.model, shape.info, shape.table
    own1 = np.arange(info["boundaries"][-1] + 100, info["boundaries"][-1] + 164)
    assert not np.isin(own1, m.prow).any()
    for kw in T.METRICS:
        lo, hi, owners, S, cutoff = tail_owners(shape, kw)
        want = m.expand_csr(S, cutoff, None, self_rows=owners)
        T.past(want[1], info)
        st = {}
        same_csr(t.neighbors(cutoff, row_begin=lo, row_end=hi, stats=st, **kwargs(kw)), want, (kw, "neighbors"))
        shape.launches("neighbors", st["launches"])
        S1 = T.score_matrix(m.take_rows(own1), m, kw)
        want = m.expand_csr(S1, 1.0, None, self_rows=own1)
        if shape.big:
            T.past(want[1], info)
        assert (np.diff(want[0].astype(np.int64)) >= shape.n // P - 2).all()
        same_csr(t.neighbors(1.0, row_begin=int(own1[0]), row_end=int(own1[-1]) + 1, **kwargs(kw)), want, (kw, "neighbors at 1.0"))


@every(ALL)
@pytest.mark.parametrize("route", [1 << 30, 0], ids=["stream", "tiles"])
def test_histogram(shape, route):
    m, info = shape.model, shape.info
    left = T.mixed_left(m, info)
    lo = info["boundaries"][-1] - 10
    own = np.arange(lo, lo + 70)
    t = shape.attach(GSIM_HIST_STREAM_MAX_ROWS=route)
    try:
        for kw in T.METRICS:
            S = T.score_matrix(left, m, kw)
            edges = T.data_edges(S)
            nb = len(edges) + 1
            want = m.expand_hist(T.hist_bins(S, edges), nb)
            assert (want > 0).sum(axis=0).min() > 0 and (not shape.big or int(want.max()) > 1 << 24), "a single count past 2^16 (2^24)"
            assert int(want[40, nb - 1]) == 1, "F against the table: the one row at 1.0 is F itself, past a boundary"
            st = {}
            hist, total = t.histogram(left, edges, stats=st, **kwargs(kw))
            shape.launches("histogram, " + ("tiles" if route == 0 else "stream"), st["tile_launches"] + st["stream_launches"])
            assert st["rows_streamed"] == (70 if route else 0) and st["rows_tiled"] == (0 if route else 70)
            assert np.array_equal(hist, want) and np.array_equal(total, want.sum(axis=0, dtype=np.uint64)), kw
            # the table against a range of itself that straddles the last boundary, the pair (row i, row i) not counted
            Sown = T.score_matrix(m.take_rows(own), m, kw)
            want = m.expand_hist(T.hist_bins(Sown, edges), nb, self_rows=own)
            hist, total = t.histogram(t, edges, row_begin=int(own[0]), row_end=int(own[-1]) + 1, exclude_self=True, **kwargs(kw))
            assert np.array_equal(hist, want) and np.array_equal(total, want.sum(axis=0, dtype=np.uint64)), (kw, "exclude_self")
    finally:
        t.close()


@every(ALL)
def test_scores(shape):
    import torch
    m, info, t = shape.model, shape.info, shape.table
    left = T.mixed_left(m, info)
    lt = shape.left_table(left)
    try:
        for kw in T.METRICS:
            S = T.score_matrix(left, m, kw)
            for lo, hi in T.straddles(m, info, 1000):
                cols = m.source_of(np.arange(lo, hi))
                want = np.ascontiguousarray(S[:, cols])
                assert (cols >= P).sum() >= 3 and float(want[40:60].max()) > 0.9, "planted columns, and family rows that meet them"
                st = {}
                got = t.scores(left, col_begin=lo, col_end=hi, stats=st, **kwargs(kw))
                shape.launches("scores", st["launches"])
                assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (kw, lo, hi, "host output")
                out = torch.full((70, hi - lo), float("nan"), dtype=torch.float32, device="cuda:0")
                assert t.scores(lt, col_begin=lo, col_end=hi, out_ptr=out.data_ptr(), **kwargs(kw)) is None
                assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (kw, lo, hi, "device output")
    finally:
        lt.close()


@every(NOT_B)
@pytest.mark.parametrize("mode", ["max", "mean"])
def test_search_group(shape, mode):
    m, info, t = shape.model, shape.info, shape.table
    queries = np.ascontiguousarray(info["family"][[0, 2, 4, 9, 13]])
    popc = T.unpack(m.sources()).sum(axis=1)
    for kw in T.METRICS:
        S = T.score_matrix(queries, m, kw)
        g, which = (S.max(0), S.argmax(0)) if mode == "max" else (T.mean_in_order(S), np.zeros(m.U, np.int64))
        cutoff = T.cutoff_between(g[:P], g[T.family_sources(m, info)])
        _, rows, s = m.expand_csr(g[None, :], cutoff, 100)
        src = m.source_of(rows)
        T.past(rows, info)
        assert len(rows) >= len(info["family"])
        hits, approx, st = t.search_group(queries, 100, capi.GROUP_MAX if mode == "max" else capi.GROUP_MEAN, cutoff, stats=True, **kwargs(kw))
        shape.launches("search_group", st["launches"])
        assert approx == int(m.multiplicities()[g >= F(cutoff)].sum()) == len(rows)
        assert np.array_equal(hits["row"], rows) and np.array_equal(bits(hits["score"]), bits(s)), (kw, mode)
        assert np.array_equal(hits["which"], which[src]) and np.array_equal(hits["popc_db"], popc[src]), (kw, mode)
