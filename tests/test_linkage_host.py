"""Complete- and average-linkage dendrograms on the host (gsim_linkage) against the rule of include/gpusim_hip.h as linkage_rule.py
restates it twice: `greedy` (the definition) and `chain` (the nearest-neighbour chain with the replay).  No GPU.  Comparisons are on
bytes; the only tolerance is against scipy's float64 average heights (1e-6: the quantisation loses less than 2^-31 a pair, the f32
result 2^-24 relative)."""
import os

import numpy as np
import pytest

import linkage_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi

KINDS = (capi.LINKAGE_COMPLETE, capi.LINKAGE_AVERAGE)
LEVELS = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)


def lattice(rng, n):
    S = LEVELS[rng.integers(0, 5, size=(n, n))]
    return np.ascontiguousarray(np.triu(S, 1) + np.triu(S, 1).T)


_ORACLE = []


def oracle_matrix():
    """the Tanimoto scores of 400 sparse 256-bit oracle rows, 100 of them copies of others: made once, never changed"""
    if not _ORACLE:
        rng = np.random.default_rng(31)
        db = O.synth_rows(0x11A6E, O.KIND_SPARSE, 0, 400, 8)
        where = rng.permutation(400)
        db[where[:100]] = db[where[100:200]]
        S = np.stack([O.tanimoto_raw(db[r], db)[0] for r in range(400)]).astype(np.float32)
        S[np.isnan(S)] = 0  # 0 / 0 is 0.0f
        S.setflags(write=False)
        _ORACLE.append(S)
    return _ORACLE[0]


def same(got, want, what):
    assert got.dtype == capi.LINKAGE_MERGE_DTYPE == R.MERGE_DTYPE
    assert got.tobytes() == want.tobytes(), (what, got[:5], want[:5])


def test_struct_layout():
    assert capi.LINKAGE_MERGE_DTYPE.itemsize == 32
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpusim_hip.h")).read()
    assert "gsim_db_linkage, THE RESULT RULE" in text and "ORDER L" in text and "GSIM_LINKAGE_MAX_ROWS 65536u" in text


def test_greedy_chain_and_the_library_agree_on_tie_heavy_matrices():
    rng = np.random.default_rng(2024)
    tied = 0
    for case in range(300):
        n = int(rng.integers(2, 41))
        S = lattice(rng, n)
        for kind in KINDS:
            want = R.greedy(S, kind)
            via_chain, scans, chain_max = R.chain(S, kind)
            got, got_scans = capi.linkage(S, kind)
            same(via_chain, want, (case, n, kind, "chain"))
            same(got, want, (case, n, kind, "library"))
            assert got_scans == scans and n - 1 <= scans <= 3 * n and chain_max <= n, (case, n, kind, got_scans, scans)
            assert (np.diff(want["score"]) <= 0).all()
            tied += len(want) - len(np.unique(want["score"]))
    assert tied > 1000  # (the cases do tie)


def test_the_oracle_matrix_with_duplicates():
    S = oracle_matrix()
    for kind in KINDS:
        want = R.greedy(S, kind)
        via_chain, scans, _ = R.chain(S, kind)
        got, got_scans = capi.linkage(S, kind)
        same(via_chain, want, (kind, "chain"))
        same(got, want, (kind, "library"))
        assert got_scans == scans
        assert (want["score"][:50] == 1.0).all() and len(np.unique(want["score"])) >= 20
        assert (np.diff(got["score"]) <= 0).all()
        assert (got["size"][-1], got["left"].max() < 2 * 400 - 1) == (400, True)
        if kind == capi.LINKAGE_AVERAGE:
            assert (got["sum_q"][:50] == 2**31).all()
        else:
            assert (got["sum_q"] == R.q(got["score"]).astype(np.uint64)).all()


def test_only_the_upper_triangle_is_read():
    rng = np.random.default_rng(5)
    S = lattice(rng, 23)
    T = S.copy()
    T[np.tril_indices(23)] = np.nan
    for kind in KINDS:
        same(capi.linkage(T, kind)[0], capi.linkage(S, kind)[0], kind)


def test_mst_cut_of_the_edges_is_the_cut_of_the_rule():
    S = oracle_matrix()
    n = len(S)
    for kind in KINDS:
        m, _ = capi.linkage(S, kind)
        edges = capi.linkage_edges(m)
        assert edges.dtype == capi.MST_EDGE_DTYPE and len(edges) == n - 1
        ncomp = []
        for t in (0.05, 0.2, 0.5, 0.8, 1.0):
            component_of, first_row, sizes = capi.mst_cut(edges, n, t)
            want = R.cut(R.greedy(S, kind), n, t)
            assert np.array_equal(component_of, want[0]) and np.array_equal(first_row, want[1]) and np.array_equal(sizes, want[2]), (kind, t)
            ncomp.append(len(first_row))
        assert ncomp == sorted(ncomp) and ncomp[0] < ncomp[-1] < n, ncomp


@pytest.mark.parametrize("method, kind", [("complete", capi.LINKAGE_COMPLETE), ("average", capi.LINKAGE_AVERAGE)])
def test_scipy_builds_the_same_tree(method, kind):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    n = 200
    rng = np.random.default_rng(77)
    vals = (rng.permutation(n * (n - 1) // 2).astype(np.float64) + 1) / (n * n)  # distinct, exact in f32: no ties
    S = np.zeros((n, n), np.float32)
    S[np.triu_indices(n, 1)] = vals
    S = S + S.T
    assert len(np.unique(S[np.triu_indices(n, 1)])) == n * (n - 1) // 2
    m, _ = capi.linkage(S, kind)
    Z = hierarchy.linkage(squareform(1.0 - S.astype(np.float64), checks=False), method)

    def leaf_sets(left, right):
        sets = {i: frozenset([i]) for i in range(n)}
        out = []
        for k in range(n - 1):
            sets[n + k] = sets[int(left[k])] | sets[int(right[k])]
            out.append(sets[n + k])
        return out

    ours, theirs = leaf_sets(m["left"], m["right"]), leaf_sets(Z[:, 0], Z[:, 1])
    assert set(ours) == set(theirs)
    height = dict(zip(theirs, Z[:, 2]))
    mine = capi.linkage_to_scipy(m, n)
    assert mine.dtype == np.float64 and mine.shape == (n - 1, 4)
    for k, s in enumerate(ours):
        if kind == capi.LINKAGE_COMPLETE:
            assert mine[k, 2] == height[s], (k, mine[k, 2], height[s])
        else:
            assert abs(mine[k, 2] - height[s]) <= 1e-6, (k, mine[k, 2], height[s])
    assert hierarchy.is_valid_linkage(mine)


def test_small_and_invalid_arguments():
    L = capi.load()
    import ctypes as C
    for kind in KINDS:
        for n in (0, 1):
            m, scans = capi.linkage(np.zeros((n, n), np.float32), kind)
            assert len(m) == 0 and scans == 0
        m, scans = capi.linkage(np.array([[0, 0.5], [0.25, 0]], np.float32), kind)
        assert len(m) == 1 and scans == 2
        assert (m["a"][0], m["b"][0], m["left"][0], m["right"][0], m["size"][0], m["score"][0], m["sum_q"][0]) == (0, 1, 0, 1, 2, 0.5, 2**30)
    S = np.full((3, 3), 0.5, np.float32)
    buf = np.zeros(2, capi.LINKAGE_MERGE_DTYPE)
    nm, scans = C.c_uint64(7), C.c_uint64(7)
    fp = S.ctypes.data_as(C.POINTER(C.c_float))

    def call(scores=fp, n=3, ld=3, kind=0, merges=buf.ctypes.data, nmerges=C.byref(nm)):
        return L.gsim_linkage(scores, n, ld, kind, merges, nmerges, C.byref(scans))

    assert call() == 0 and nm.value == 2
    assert call(nmerges=None) == -1
    assert call(scores=None) == -1 and nm.value == 0
    assert call(merges=None) == -1
    assert call(ld=2) == -1
    assert call(kind=2) == -1 and call(kind=-1) == -1
    assert call(n=capi.LINKAGE_MAX_ROWS + 1, ld=capi.LINKAGE_MAX_ROWS + 1) == -1 and b"65536" in L.gsim_last_error()
    for bad in (np.nan, -0.25, 1.5, np.inf):
        T = S.copy()
        T[0, 2] = bad
        assert L.gsim_linkage(T.ctypes.data_as(C.POINTER(C.c_float)), 3, 3, 0, buf.ctypes.data, C.byref(nm), None) == -1, bad
        T = S.copy()
        T[2, 0] = bad  # (the lower triangle is not read)
        assert L.gsim_linkage(T.ctypes.data_as(C.POINTER(C.c_float)), 3, 3, 1, buf.ctypes.data, C.byref(nm), None) == 0, bad
    with pytest.raises(capi.GsimError):
        capi.linkage(np.zeros((2, 3), np.float32), 0)
    with pytest.raises(capi.GsimError):
        capi.linkage_to_scipy(buf, 5)


def test_the_device_call_checks_its_arguments_before_any_device_state():
    """every GSIM_ERR_INVALID case of gsim_db_linkage on a table that is not on a GPU, then GSIM_ERR_STATE for that"""
    L = capi.load()
    import ctypes as C
    t = capi.Table(256).add_rows(np.ones((5, 8), np.uint32))
    buf = np.zeros(4, capi.LINKAGE_MERGE_DTYPE)
    nm = C.c_uint64(9)

    def call(db=t._h, b=0, e=5, kind=0, metric=capi.METRIC_TANIMOTO, alpha=1.0, beta=1.0, merges=buf.ctypes.data, nmerges=C.byref(nm)):
        return L.gsim_db_linkage(db, b, e, kind, metric, alpha, beta, 0, merges, nmerges, None)

    assert call(db=None) == -1 and call(nmerges=None) == -1
    assert call(b=3, e=2) == -1 and call(e=6) == -1
    assert call(kind=2) == -1 and b"unknown linkage" in L.gsim_last_error()
    assert call(metric=7) == -1
    TV = capi.METRIC_TVERSKY
    assert call(metric=TV, alpha=0.3, beta=0.7) == -1
    assert call(metric=TV, alpha=-1.0, beta=-1.0) == -1 and call(metric=TV, alpha=np.inf, beta=np.inf) == -1
    assert call(metric=TV, alpha=np.nan, beta=np.nan) == -1
    assert call(merges=None) == -1
    assert call(b=2, e=2) == 0 and nm.value == 0
    assert call(b=2, e=3, merges=None) == 0 and nm.value == 0
    assert call() == -5 and nm.value == 0  # not finalized: GSIM_ERR_STATE
    assert call(metric=TV, alpha=0.5, beta=0.5) == -5
    wide = capi.Table(8192).add_rows(np.ones((3, 256), np.uint32))
    assert call(db=wide._h, e=3) == -1 and b"4096" in L.gsim_last_error()
    big = capi.Table(32).add_rows(np.ones((capi.LINKAGE_MAX_ROWS + 2, 1), np.uint32))
    huge = np.zeros(capi.LINKAGE_MAX_ROWS + 1, capi.LINKAGE_MERGE_DTYPE)
    assert call(db=big._h, e=capi.LINKAGE_MAX_ROWS + 1, merges=huge.ctypes.data) == -1 and b"65536" in L.gsim_last_error()
    assert call(db=big._h, b=2, e=capi.LINKAGE_MAX_ROWS + 2, merges=huge.ctypes.data) == -5
    with pytest.raises(capi.GsimError) as e:
        t.linkage(capi.LINKAGE_AVERAGE)
    assert e.value.code == -5
