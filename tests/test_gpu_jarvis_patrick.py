"""Jarvis-Patrick clustering and shared-nearest-neighbour graphs on the GPU (gsim_db_snn, gsim_db_jarvis_patrick).

Expected values: the oracle gives the pair scores (test_gpu_components.score_matrix, as tests/test_gpu_linkage.py builds its matrix),
knn_rule.knn_rule turns them into the lists, and jarvis_patrick_rule -- Python sets, written from include/gpusim_hip.h's contract --
gives the counts, the partitions and the reproducible stats.  Indices, counts and labels are compared as bytes: no tolerances.

Tables: test_gpu_knn.planted(seed, KIND_MORGAN, 1200, W) at 1024 bits (seed 0x7A31) and at 160 bits (a padded width, seed 0x7A16):
four full 256-row tiles and one of 176 rows, seven duplicates and one all-zero row; one dense 700-row and one sparse 1200-row table for
the counts only.  k runs over the lane-group edges {1, 2, 15, 16, 17, 63, 64, 65, 127, 128}.

NON-VACUITY is asserted on the expected result, never on the code under test: every compared level on the Morgan tables has at least
10 clusters of two or more rows and at least 10 singletons.  The ladders were chosen on the CPU from the rule; what it gives there
(clusters of two or more rows / singletons), smallest positive cutoff unless stated:
  1024 bits, open, mutual   k = 1: kmin 0: 124 / 952.   k = 2: 0, 1: 142 / 816, 107 / 934.
                            k = 15: 0, 1, 2, 3, 6, 8, 11, 14: 17 / 129, 24 / 158, 42 / 219, 51 / 321, 63 / 542, 68 / 610, 82 / 785, 46 / 1080.
                            k = 16: 3, 6, 8, 15: 41 / 284, 61 / 522, 65 / 591, 49 / 1077; 0, 1, 2, 4, 7, 9, 12, 15: 13 / 114, 21 / 140,
                            37 / 194, 51 / 383, 64 / 557, 68 / 622, 72 / 847, 49 / 1077.   k = 17: 3, 8, 12, 16: 34 / 254, 62 / 579, 80 / 778, 44 / 1085.
                            k = 63: 30, 32, 47, 62: 55 / 557, 57 / 579, 59 / 926, 33 / 1125.   k = 64: 31, 33, 48, 63: 54 / 567, 56 / 583,
                            58 / 933, 33 / 1125; 32 alone: 56 / 576.   k = 65: 31, 33, 48, 64: 55 / 556, 56 / 580, 56 / 917, 33 / 1125.
                            k = 127: 62, 64, 95, 126: 40 / 512, 48 / 530, 69 / 887, 33 / 1125.   k = 128: 63, 65, 96, 127: 43 / 513, 48 / 536,
                            69 / 891, 33 / 1125 (kmin <= 6 at k = 128 collapses to one cluster and is not a compared level).
  1024 bits, k = 16         EITHER 4, 8, 12, 15: 20 / 134, 58 / 545, 72 / 832, 46 / 1049.   CLOSED 3, 9, 14, 17: 21 / 140, 64 / 557, 72 / 847,
                            49 / 1077.   CLOSED | EITHER 7, 9, 12, 17: 45 / 361, 58 / 519, 68 / 654, 49 / 1077.
  1024 bits, k = 128        EITHER 63, 65, 96, 127: 41 / 509, 47 / 531, 69 / 891, 33 / 1125.   CLOSED 63, 65, 96, 129: 36 / 483, 43 / 513, 69 / 856,
                            33 / 1125.   CLOSED | EITHER 63, 65, 96, 129: 34 / 481, 42 / 509, 69 / 856, 33 / 1125.
  1024 bits, k = 16, cutoff 0.3 (1110 of 1200 lists shorter than k)   open 3, 6, 8, 15: 64 / 616, 43 / 764, 22 / 954, 13 / 1157.
                            EITHER 3, 6, 8, 15: 64 / 601, 43 / 749, 22 / 939, 10 / 1129.
  1024 bits, k = 16, Tversky 0.5 / 0.5   3, 6, 8, 15: 41 / 284, 61 / 522, 65 / 591, 49 / 1077.
  1024 bits, k = 16, Tversky 0.9 / 0.1   3, 6, 8, 15: 50 / 300, 60 / 486, 65 / 558, 47 / 1090; EITHER 4, 8, 12, 15: 15 / 171, 63 / 507, 67 / 860, 46 / 1073.
  160 bits, k = 16          open 3, 6, 8, 15: 82 / 387, 42 / 602, 37 / 636, 61 / 1041.   EITHER 4, 8, 12, 15: 24 / 240, 28 / 551, 27 / 649, 63 / 992.
                            CLOSED 3, 9, 14, 17: 34 / 158, 36 / 627, 40 / 713, 61 / 1041.   CLOSED | EITHER 7, 9, 12, 17: 27 / 425, 27 / 542,
                            29 / 618, 61 / 1041."""
import ctypes as C

import numpy as np
import pytest

import jarvis_patrick_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi
from gpusimilarity_amd.fingerprintdb import FingerprintDB
from knn_rule import knn_rule
from test_gpu_components import score_matrix
from test_gpu_knn import COL_TILE, TINY, as_bytes, planted, table

pytestmark = pytest.mark.gpu
N = 1200
TAN = dict()
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
TVA = dict(metric=capi.METRIC_TVERSKY, alpha=0.9, beta=0.1)
OPEN, EITHER, CLOSED, BOTH = dict(), dict(either=True), dict(closed=True), dict(closed=True, either=True)
SEEDS = {1024: 0x7A31, 160: 0x7A16}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rows_of(bits):
    def make():
        db = planted(SEEDS[bits], O.KIND_MORGAN, N, bits // 32)
        db.setflags(write=False)
        return db
    return cached(("db", bits), make)


def name_of(kw):
    return tuple(sorted(kw.items()))


def lists_of(bits, k, cutoff=TINY, kw=TAN):
    """the expected CSR of gsim_db_knn on the Morgan table of that width: the oracle's scores through knn_rule; computed once"""
    S = cached(("S", bits, name_of(kw)), lambda: score_matrix(rows_of(bits), kw))
    return cached(("csr", bits, k, cutoff, name_of(kw)), lambda: knn_rule(S, k, cutoff))


def entries_of(csr, closed=False):
    """jarvis_patrick_rule.entries_of for an expected CSR: computed once per CSR object (the cache keeps them alive) and convention"""
    return cached(("entries", id(csr), bool(closed)), lambda: (csr, R.entries_of(csr[0], csr[1], closed)))[1]


def levels_of(csr, kmins, flags):
    want = R.jarvis_patrick_rule(csr[0], csr[1], kmins, entries=entries_of(csr, flags.get("closed")), **flags)
    for kmin, level in zip(kmins, want):
        multi, single = R.multi(level)
        assert multi >= 10 and single >= 10, ("a vacuous level", kmin, flags, multi, single)
    return want


def same_levels(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        for x, y, part in zip(g, w, ("cluster_of", "first_row", "sizes")):
            assert x.dtype == np.uint32 and x.tobytes() == y.tobytes(), (what, l, part)


def same_stats(st, csr, kmins, flags, what):
    want = R.stats_rule(csr[0], csr[1], kmins, entries=entries_of(csr, flags.get("closed")), **flags)
    assert st["rows"] == len(csr[0]) - 1 and st["entries"] == want["entries"] and st["mutual_entries"] == want["mutual_entries"], (what, st, want)
    assert st["links"][:len(kmins)] == want["links"] and not any(st["links"][len(kmins):]), (what, st["links"], want["links"])
    assert st["unions"] == want["unions"], (what, st["unions"], want["unions"])
    assert st["pairs"] == st["rows"] ** 2 and st["launches"] >= 1 and st["knn_ms"] > 0 and st["link_ms"] > 0 and st["clock_mhz"] > 100, (what, st)


def check_table(t, csr, k, cutoff, kw, kmins, flags, what):
    """gsim_db_snn and gsim_db_jarvis_patrick on an open table against the rule on the expected lists `csr`"""
    knn = t.knn(k, cutoff, **kw)
    assert as_bytes(knn) == as_bytes(csr), (what, "the lists themselves")
    for closed in (False, True):
        st = {}
        got = t.snn(k, cutoff, closed=closed, stats=st, **kw)
        assert as_bytes(got[:3]) == as_bytes(knn), (what, "gsim_db_snn's CSR is gsim_db_knn's")
        want = R.snn_rule(csr[0], csr[1], closed, entries=entries_of(csr, closed))
        assert got[3].dtype == np.uint32 and got[3].tobytes() == want.tobytes(), (what, closed, "shared")
        assert got[3].tobytes() == capi.snn(knn[0], knn[1], closed=closed).tobytes()
        assert st["entries"] == len(want) and st["mutual_entries"] == int((want >> 31).sum()) and st["k"] == k and not any(st["links"]), (what, st)
    want = levels_of(csr, kmins, flags)
    got, st = t.jarvis_patrick(k, kmins, cutoff, **kw, **flags)
    same_levels(got, want, what)
    same_levels(capi.jarvis_patrick(knn[0], knn[1], kmins, **flags), want, (what, "the host function on gsim_db_knn's CSR"))
    same_stats(st, csr, kmins, flags, what)
    for a, b in zip(want, want[1:]):  # level l + 1 refines level l
        assert len(set(zip(a[0].tolist(), b[0].tolist()))) == len(b[1])
    return got


LADDERS = {1: [0], 2: [0, 1], 15: [0, 1, 2, 3, 6, 8, 11, 14], 16: [3, 6, 8, 15], 17: [3, 8, 12, 16], 63: [30, 32, 47, 62], 64: [31, 33, 48, 63],
           65: [31, 33, 48, 64], 127: [62, 64, 95, 126], 128: [63, 65, 96, 127]}


@pytest.mark.parametrize("k", sorted(LADDERS))
def test_parity_with_the_rule_at_the_lane_group_edges(k):
    t = table(rows_of(1024))
    check_table(t, lists_of(1024, k), k, TINY, TAN, LADDERS[k], OPEN, k)
    t.close()


FLAG_CASES = [(1024, 16, EITHER, [4, 8, 12, 15]), (1024, 16, CLOSED, [3, 9, 14, 17]), (1024, 16, BOTH, [7, 9, 12, 17]),
              (1024, 128, EITHER, [63, 65, 96, 127]), (1024, 128, CLOSED, [63, 65, 96, 129]), (1024, 128, BOTH, [63, 65, 96, 129]),
              (160, 16, OPEN, [3, 6, 8, 15]), (160, 16, EITHER, [4, 8, 12, 15]), (160, 16, CLOSED, [3, 9, 14, 17]), (160, 16, BOTH, [7, 9, 12, 17])]


@pytest.mark.parametrize("bits,k,flags,kmins", FLAG_CASES)
def test_the_four_flag_combinations(bits, k, flags, kmins):
    t = table(rows_of(bits))
    check_table(t, lists_of(bits, k), k, TINY, TAN, kmins, flags, (bits, k, flags))
    t.close()


def test_a_biting_cutoff_leaves_most_lists_short():
    k, cutoff = 16, 0.3
    csr = lists_of(1024, k, cutoff)
    assert int((np.diff(csr[0].astype(np.int64)) < k).sum()) == 1110
    t = table(rows_of(1024))
    check_table(t, csr, k, cutoff, TAN, [3, 6, 8, 15], OPEN, "cutoff 0.3")
    check_table(t, csr, k, cutoff, TAN, [3, 6, 8, 15], EITHER, "cutoff 0.3, either")
    t.close()


@pytest.mark.parametrize("kw,flags,kmins", [(TV, OPEN, [3, 6, 8, 15]), (TVA, OPEN, [3, 6, 8, 15]), (TVA, EITHER, [4, 8, 12, 15])])
def test_tversky(kw, flags, kmins):
    k = 16
    csr = lists_of(1024, k, TINY, kw)
    if kw is TVA:
        assert as_bytes(csr) != as_bytes(lists_of(1024, k)), "asymmetric weights change the lists"
    t = table(rows_of(1024))
    check_table(t, csr, k, TINY, kw, kmins, flags, (kw, flags))
    t.close()


def test_ladders_of_one_four_and_eight_levels_and_their_stripes():
    k, eight = 16, [0, 1, 2, 4, 7, 9, 12, 15]
    csr = lists_of(1024, k)
    t = table(rows_of(1024))
    want = levels_of(csr, eight, OPEN)
    got, st = t.jarvis_patrick(k, eight, TINY)
    same_levels(got, want, "eight levels")
    same_stats(st, csr, eight, OPEN, "eight levels")
    four, _ = t.jarvis_patrick(k, [2, 7, 9, 15], TINY)
    same_levels(four, [want[2], want[4], want[5], want[7]], "four levels")
    for l, kmin in enumerate(eight):  # a single-level call equals the matching stripe
        one, st1 = t.jarvis_patrick(k, kmin, TINY)
        same_levels(one, [got[l]], ("single level", kmin))
        assert st1["unions"] == N - len(got[l][1]) and st1["links"][0] == st["links"][l]
    alone, _ = t.jarvis_patrick(64, [32], TINY)
    same_levels(alone, levels_of(lists_of(1024, 64), [32], OPEN), "k = 64, one level")
    # first_row and sizes may be left out
    bare, _ = t.jarvis_patrick(k, eight, TINY, first_row=False, sizes=False)
    assert all(f is None and s is None and c.tobytes() == w[0].tobytes() for (c, f, s), w in zip(bare, want))
    t.close()


def test_twice_and_two_launch_cuts():
    k, kmins = 16, [3, 6, 8, 15]
    db = rows_of(1024)
    whole = table(db)
    a, st0 = whole.jarvis_patrick(k, kmins, TINY)
    b, _ = whole.jarvis_patrick(k, kmins, TINY)
    s0 = whole.snn(k, TINY)
    assert as_bytes(whole.snn(k, TINY)) == as_bytes(s0), "byte-identical from run to run"
    whole.close()
    same_levels(b, a, "byte-identical from run to run")
    same_levels(a, levels_of(lists_of(1024, k), kmins, OPEN), "default plan")
    ntiles = -(-N // COL_TILE)
    for pairs, launches in ((1, ntiles), (N * 2 * COL_TILE, -(-ntiles // 2))):
        cut = table(db, pairs=pairs)
        c, st = cut.jarvis_patrick(k, kmins, TINY)
        assert st["launches"] == launches > st0["launches"], (st, st0)
        same_levels(c, a, pairs)
        assert [st[f] for f in ("entries", "mutual_entries", "links", "unions", "inserts")] == \
               [st0[f] for f in ("entries", "mutual_entries", "links", "unions", "inserts")]
        assert as_bytes(cut.snn(k, TINY)) == as_bytes(s0), pairs
        cut.close()


def test_the_row_base_shows_in_indices_and_first_row_only():
    k, kmins, base = 16, [3, 6, 8, 15], 7000
    csr = lists_of(1024, k)
    plain = table(rows_of(1024))
    p_levels, _ = plain.jarvis_patrick(k, kmins, TINY)
    p_snn = plain.snn(k, TINY)
    plain.close()
    t = table(rows_of(1024), base=base)
    levels, _ = t.jarvis_patrick(k, kmins, TINY)
    for (c, f, s), (pc, pf, ps) in zip(levels, p_levels):
        assert c.tobytes() == pc.tobytes() and s.tobytes() == ps.tobytes() and np.array_equal(f, pf + np.uint32(base))
    got = t.snn(k, TINY)
    assert np.array_equal(got[0], p_snn[0]) and np.array_equal(got[1], p_snn[1] + np.uint32(base))
    assert got[2].tobytes() == p_snn[2].tobytes() and got[3].tobytes() == p_snn[3].tobytes()
    based = (csr[0], csr[1] + np.uint32(base), csr[2])
    same_levels(levels, R.jarvis_patrick_rule(based[0], based[1], kmins, row_base=base), "the rule with the base")
    t.close()


def test_counts_on_a_dense_and_a_sparse_table():
    for kind, n, W, k in ((O.KIND_DENSE, 700, 8, 16), (O.KIND_DENSE, 700, 8, 100), (O.KIND_SPARSE, 1200, 32, 16), (O.KIND_SPARSE, 1200, 32, 40)):
        db = cached(("plain", kind, n, W), lambda: planted(0x7A00 + kind, kind, n, W))
        S = cached(("plainS", kind, n, W), lambda: score_matrix(db))
        csr = knn_rule(S, k, TINY)
        t = table(db)
        for closed in (False, True):
            got = t.snn(k, TINY, closed=closed)
            assert as_bytes(got[:3]) == as_bytes(csr), (kind, k)
            want = R.snn_rule(csr[0], csr[1], closed)
            assert got[3].tobytes() == want.tobytes(), (kind, k, closed)
        assert len(np.unique(want & 0x7FFFFFFF)) >= 5 and 0 < int((want >> 31).sum()) < len(want)
        t.close()


def test_the_graph_object_and_the_wrapper():
    """gsim_db_snn's result is a gsim_graph of its own kind: the other kinds' accessors refuse it, and its accessors refuse them."""
    n, k = 300, 5
    db = np.ascontiguousarray(rows_of(1024)[:n])
    t = table(db)
    L = capi.load()
    g = C.c_void_p()
    assert L.gsim_db_snn(t._h, k, TINY, 0, 1.0, 1.0, 0, C.byref(g)) == 0 and g.value
    js, gs, ks, kj, ss = capi.GsimJoinStats(), capi.GsimGraphStats(), capi.GsimKnnStats(), capi.GsimKnnJoinStats(), capi.GsimSnnStats()
    assert L.gsim_graph_get_join_stats(g, C.byref(js)) == -1 and L.gsim_graph_get_knn_stats(g, C.byref(ks)) == -1
    assert L.gsim_graph_get_knn_join_stats(g, C.byref(kj)) == -1
    assert L.gsim_graph_get_stats(g, C.byref(gs)) == 0 and L.gsim_graph_get_snn_stats(g, C.byref(ss)) == 0
    rows, nnz = C.c_uint64(0), C.c_uint64(0)
    assert L.gsim_graph_shape(g, C.byref(rows), C.byref(nnz)) == 0 and rows.value == n
    assert gs.launches == ss.launches >= 1 and gs.pairs == ss.entries == nnz.value and ss.rows == n and ss.k == k and ss.pairs == n * n
    assert ss.knn_ms > 0 and ss.sort_ms > 0 and ss.link_ms > 0 and ss.wall_ms > 0 and ss.clock_mhz > 100
    assert L.gsim_graph_copy_shared(g, None) == -1
    L.gsim_graph_destroy(g)
    kn = C.c_void_p()
    assert L.gsim_db_knn(t._h, k, TINY, 0, 1.0, 1.0, 0, n, C.byref(kn)) == 0
    buf = np.zeros(n * k, np.uint32)
    assert L.gsim_graph_copy_shared(kn, buf.ctypes.data_as(C.POINTER(C.c_uint32))) == -1 and L.gsim_graph_get_snn_stats(kn, C.byref(ss)) == -1
    L.gsim_graph_destroy(kn)
    want, _ = t.jarvis_patrick(k, [2], TINY)
    t.close()
    fdb = FingerprintDB(1024, n, "k", [db], [b"s%d" % i for i in range(n)], [b"i%d" % i for i in range(n)])
    fdb.copyToGPU()
    clusters = fdb.jarvis_patrick(k, 2)
    cluster_of, first_row, sizes = want[0]
    assert [c[0] for c in clusters] == first_row.tolist() and [len(c) for c in clusters] == sizes.tolist()
    assert all(list(c) == np.flatnonzero(cluster_of == x).tolist() for x, c in enumerate(clusters))


def test_the_search_state_is_left_as_it_was():
    k, kmins = 16, [3, 6, 8, 15]
    db = rows_of(1024)
    t = table(db)
    t.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 600, N - 1]])

    def searches():
        hits, approx = t.search(q, 50, 0.4)
        bufs = (np.zeros((len(q), 50), capi.HIT_DTYPE), np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint64))
        t.search_each_into(q, 50, bufs, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes() + b"".join(bufs[0][i, :bufs[1][i]].tobytes() for i in range(len(q))) + bufs[2].tobytes()

    before = searches()
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0 = t.timing()
    got, _ = t.jarvis_patrick(k, kmins, TINY)
    shared = t.snn(k, TINY)
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    with pytest.raises(capi.GsimError) as e:
        t.jarvis_patrick(k, [17], TINY)  # a failed call ...
    assert e.value.code == -1
    again, _ = t.jarvis_patrick(k, kmins, TINY)  # ... and a correct one right after it
    same_levels(again, got, "after a failed call")
    assert as_bytes(t.snn(k, TINY)) == as_bytes(shared)
    assert searches() == before
    same_levels(got, levels_of(lists_of(1024, k), kmins, OPEN), "between the searches")
    t.close()


def test_generated_and_attached_tables():
    import torch
    n, W, k, seed, kmins = 1500, 5, 16, 0x7A0C, [3, 8, 15]
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    csr = knn_rule(score_matrix(db), k, TINY)
    want = R.jarvis_patrick_rule(csr[0], csr[1], kmins)
    shared = R.snn_rule(csr[0], csr[1])
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    same_levels(g.jarvis_patrick(k, kmins, TINY)[0], want, "generated")
    got = g.snn(k, TINY)
    assert as_bytes(got[:3]) == as_bytes(csr) and got[3].tobytes() == shared.tobytes()
    g.close()
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), n, 0)
    same_levels(a.jarvis_patrick(k, kmins, TINY)[0], want, "attached (160 bits: a zero-padded copy)")
    got = a.snn(k, TINY)
    assert as_bytes(got[:3]) == as_bytes(csr) and got[3].tobytes() == shared.tobytes()
    a.close()
    del ten


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_tiny_tables(n):
    k = 16
    db = np.ascontiguousarray(rows_of(1024)[:max(n, 1)])
    if n == 5:
        db = db.copy()
        db[3] = db[0]  # a duplicate pair
    if n == 0:  # (a table without rows is on no GPU: the clustering is empty, the graph call is gsim_db_knn's state error)
        t = capi.Table(1024)
        levels, st = t.jarvis_patrick(k, [0, 1], TINY)
        assert all(len(c) == 0 and len(f) == 0 and len(s) == 0 for c, f, s in levels) and st["rows"] == 0
        with pytest.raises(capi.GsimError) as e:
            t.snn(k, TINY)
        assert e.value.code == -5
        t.close()
        return
    t = table(db)
    t.set_row_base(100)
    levels, st = t.jarvis_patrick(k, [0, 1], TINY)
    got = t.snn(k, TINY)
    if n < 2:
        assert got[0].tolist() == [0] * (n + 1) and len(got[1]) == 0 and len(got[3]) == 0
        for c, f, s in levels:
            assert c.tolist() == [0] * n and f.tolist() == [100] * n and s.tolist() == [1] * n
    else:
        csr = knn_rule(score_matrix(db), k, TINY, row_base=100)
        assert as_bytes(got[:3]) == as_bytes(csr) and got[3].tobytes() == R.snn_rule(csr[0], csr[1], row_base=100).tobytes()
        same_levels(levels, R.jarvis_patrick_rule(csr[0], csr[1], [0, 1], row_base=100), n)
        assert len(levels[0][1]) < n, "some rows are joined"
    t.close()


def test_contention_on_identical_rows():
    """4096 identical rows, k = 8: every list is the lowest eight other rows.  Mutual: rows 0 .. 8 are one cluster and every other row
    a singleton; EITHER: every entry links its owner to one of rows 0 .. 8 -- 32 768 unions into one tree."""
    n, k = 4096, 8
    db = np.tile(rows_of(1024)[5], (n, 1))
    lists = [[j for j in range(9) if j != i][:k] for i in range(n)]
    indptr = np.arange(n + 1, dtype=np.uint64) * k
    indices = np.array(lists, np.uint32).reshape(-1)
    t = table(db)
    knn = t.knn(k, TINY)
    assert np.array_equal(knn[0], indptr) and np.array_equal(knn[1], indices)
    got = t.snn(k, TINY)
    assert got[3].tobytes() == R.snn_rule(indptr, indices).tobytes()
    for flags, kmins in ((OPEN, [0, 7]), (EITHER, [0, 6]), (BOTH, [0, 8])):
        want = R.jarvis_patrick_rule(indptr, indices, kmins, **flags)
        levels, st = t.jarvis_patrick(k, kmins, TINY, **flags)
        same_levels(levels, want, flags)
        same_stats(st, (indptr, indices), kmins, flags, flags)
    mutual = R.jarvis_patrick_rule(indptr, indices, [0])[0]
    assert mutual[2].tolist() == [9] + [1] * (n - 9)
    assert R.jarvis_patrick_rule(indptr, indices, [0], either=True)[0][2].tolist() == [n]
    t.close()
