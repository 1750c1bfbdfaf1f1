"""CPU checks of the neighbour-list / Butina entry points: gsim_butina (host code) against a short restatement of the rule
in include/gpusim_hip.h, and argument validation of gsim_db_neighbors without a GPU -- errors, never a CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from gpusimilarity_amd import capi


def butina_rule(indptr, indices):
    """The rule as the header states it: candidates by (count desc, row desc); skip assigned ones; a centroid takes
    itself and its unassigned neighbours; cluster ids in creation order."""
    n = len(indptr) - 1
    order = sorted(range(n), key=lambda r: (int(indptr[r + 1] - indptr[r]), r), reverse=True)
    cluster_of = [None] * n
    centroids = []
    for r in order:
        if cluster_of[r] is not None:
            continue
        cluster_of[r] = len(centroids)
        for j in indices[indptr[r]:indptr[r + 1]]:
            if cluster_of[j] is None:
                cluster_of[j] = len(centroids)
        centroids.append(r)
    return np.array(cluster_of, dtype=np.uint32), np.array(centroids, dtype=np.uint32)


def csr_from_pairs(n, pairs):
    lists = [set() for _ in range(n)]
    for i, j in pairs:
        if i != j:
            lists[i].add(j)
            lists[j].add(i)
    indptr = np.zeros(n + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum([len(x) for x in lists])
    indices = np.array([j for x in lists for j in sorted(x)], dtype=np.uint32)
    return indptr, indices


@pytest.mark.parametrize("seed", range(12))
def test_butina_matches_the_stated_rule_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 300))
    m = int(rng.integers(0, 4 * n))
    pairs = rng.integers(0, n, size=(m, 2))
    indptr, indices = csr_from_pairs(n, pairs)
    got_c, got_k = capi.butina(indptr, indices)
    want_c, want_k = butina_rule(indptr, indices)
    assert (got_c == want_c).all() and (got_k == want_k).all()
    # every row is in exactly one cluster, and every member is its centroid's neighbour
    assert len(set(got_k.tolist())) == len(got_k)
    for r in range(n):
        c = got_c[r]
        k = got_k[c]
        assert r == k or r in set(indices[indptr[k]:indptr[k + 1]].tolist())


def test_butina_ties_break_by_row_index_descending():
    # 0-1, 2-3: all counts equal -> candidates 3, 2, 1, 0: clusters {3, 2}, {1, 0}
    indptr, indices = csr_from_pairs(4, [(0, 1), (2, 3)])
    c, k = capi.butina(indptr, indices)
    assert list(k) == [3, 1] and list(c) == [1, 1, 0, 0]
    # a path 0-1-2-3-4: rows 1, 2, 3 have two neighbours -> 3 first (takes 2, 4), then 1 (takes 0)
    indptr, indices = csr_from_pairs(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    c, k = capi.butina(indptr, indices)
    assert list(k) == [3, 1] and list(c) == [1, 1, 0, 0, 0]
    # a star around 0 beats a higher row index; isolated rows become singletons, highest row first
    indptr, indices = csr_from_pairs(7, [(0, 1), (0, 2), (0, 3), (4, 5)])
    c, k = capi.butina(indptr, indices)
    assert list(k) == [0, 5, 6] and list(c) == [0, 0, 0, 0, 1, 1, 2]
    # no rows at all
    c, k = capi.butina(np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert len(c) == 0 and len(k) == 0


def test_butina_rejects_malformed_graphs():
    with pytest.raises(capi.GsimError) as e:
        capi.butina(np.array([1, 2], np.uint64), np.array([0, 0], np.uint32))
    assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        capi.butina(np.array([0, 2, 1], np.uint64), np.array([1, 0], np.uint32))
    assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        capi.butina(np.array([0, 1, 2], np.uint64), np.array([1, 2], np.uint32))  # column 2 of a 2-row graph
    assert e.value.code == -1
    L = capi.load()
    assert L.gsim_butina(None, None, 0, None, None, None) == -1


def test_neighbors_argument_validation_without_a_gpu():
    t = capi.Table(1024).add_rows(np.arange(4 * 32, dtype=np.uint32).reshape(4, 32))
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(capi.GsimError) as e:
            t.neighbors(bad)
        assert e.value.code == -1, bad
    with pytest.raises(capi.GsimError) as e:
        t.neighbors(0.5, metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7)  # asymmetric
    assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        t.neighbors(0.5, metric=7)
    assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        t.neighbors(0.5, row_begin=3, row_end=2)
    assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        t.neighbors(0.5, row_begin=0, row_end=5)
    assert e.value.code == -1
    # valid arguments, but the rows are not on a GPU: a state error, never a host computation
    for kw in ({}, dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5), dict(row_begin=1, row_end=3)):
        with pytest.raises(capi.GsimError) as e:
            t.neighbors(0.5, **kw)
        assert e.value.code == -5, kw
    wide = capi.Table(4096 + 32).add_rows(np.zeros((2, 129), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        wide.neighbors(0.5)
    assert e.value.code == -1
    L = capi.load()
    g = C.c_void_p(123)
    assert L.gsim_db_neighbors(None, 0.5, 0, 1.0, 1.0, 0, 0, C.byref(g)) == -1
    assert L.gsim_db_neighbors(t._h, 0.5, 0, 1.0, 1.0, 0, 4, None) == -1
    assert L.gsim_graph_shape(None, None, None) == -1
    assert L.gsim_graph_copy(None, None, None, None) == -1
    assert L.gsim_graph_get_stats(None, None) == -1
    assert L.gsim_graph_destroy(None) == 0
