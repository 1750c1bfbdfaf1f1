"""The rule of gsim_db_snn / gsim_db_jarvis_patrick and their host companions (include/gpusim_hip.h), restated with Python sets over
a CSR of lists.  Written from the contract, not from the C++.

L(i) is the set of rows in list i.  shared(i, j) = |L(i) & L(j)|, with `closed` + [j in L(i)] + [i in L(j)]; mutual(i, j): j in L(i)
and i in L(j).  A pair {i, j}, i != j, is a link at a level when it is mutual -- with `either`: j in L(i) or i in L(j) -- and
shared(i, j) >= the level's kmin.  The clusters of a level are the connected components of its links, numbered in ascending order of
their smallest row."""
import numpy as np

MUTUAL_BIT = 0x80000000


def lists_of(indptr, indices, row_base=0):
    indptr = np.asarray(indptr).astype(np.int64)
    indices = np.asarray(indices).astype(np.int64) - row_base
    return [set(indices[indptr[r]:indptr[r + 1]].tolist()) for r in range(len(indptr) - 1)]


def shared_of(L, i, j, closed=False):
    return len(L[i] & L[j]) + (int(j in L[i]) + int(i in L[j]) if closed else 0)


def entries_of(indptr, indices, closed=False, row_base=0):
    """every entry e = (i, j) of the CSR, in its order, with shared(i, j) and whether i is in list j: [(i, j, shared, mutual)]"""
    L = lists_of(indptr, indices, row_base)
    indptr = np.asarray(indptr).astype(np.int64)
    cols = (np.asarray(indices).astype(np.int64) - row_base).tolist()
    return [(i, cols[e], shared_of(L, i, cols[e], closed), i in L[cols[e]]) for i in range(len(L)) for e in range(indptr[i], indptr[i + 1])]


def snn_rule(indptr, indices, closed=False, row_base=0, entries=None):
    """-> shared uint32 [nnz]: per entry e = (i, j), shared(i, j) | (MUTUAL_BIT where i is in list j)"""
    entries = entries_of(indptr, indices, closed, row_base) if entries is None else entries
    return np.array([s | (MUTUAL_BIT if mutual else 0) for _, _, s, mutual in entries], np.int64).astype(np.uint32)


def links_of(entries, kmin, either=False):
    """the set of pairs (i, j), i < j, that are links at kmin"""
    return {(min(i, j), max(i, j)) for i, j, s, mutual in entries if i != j and (mutual or either) and s >= kmin}


def number(n, links):
    """union-find over the links -> (cluster_of uint32 [n], first_row uint32 [nc], sizes uint32 [nc])"""
    parent = list(range(n))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in links:
        x, y = root(i), root(j)
        if x != y:
            parent[max(x, y)] = min(x, y)
    cluster_of = np.zeros(n, np.uint32)
    first, sizes = [], []
    for r in range(n):  # ascending: a cluster's smallest row is met first and takes the next number
        x = root(r)
        if x == r:
            cluster_of[r] = len(first)
            first.append(r)
            sizes.append(1)
        else:
            cluster_of[r] = cluster_of[x]
            sizes[cluster_of[x]] += 1
    return cluster_of, np.array(first, np.uint32), np.array(sizes, np.uint32)


def jarvis_patrick_rule(indptr, indices, kmins, closed=False, either=False, row_base=0, entries=None):
    """-> one (cluster_of, first_row (+ row_base), sizes) per kmin"""
    n = len(indptr) - 1
    entries = entries_of(indptr, indices, closed, row_base) if entries is None else entries
    out = []
    for kmin in np.atleast_1d(kmins).tolist():
        c, f, s = number(n, links_of(entries, int(kmin), either))
        out.append((c, f + np.uint32(row_base), s))
    return out


def stats_rule(indptr, indices, kmins, closed=False, either=False, row_base=0, entries=None):
    """the reproducible fields of gsim_snn_stats: entries, mutual_entries, links[l] (entries meeting level l's condition), unions"""
    n = len(indptr) - 1
    entries = entries_of(indptr, indices, closed, row_base) if entries is None else entries
    links, unions = [], 0
    for kmin in np.atleast_1d(kmins).tolist():
        links.append(sum(1 for _, _, s, mutual in entries if (mutual or either) and s >= kmin))
        unions += n - len(number(n, links_of(entries, int(kmin), either))[1])
    return dict(entries=len(entries), mutual_entries=sum(1 for e in entries if e[3]), links=links, unions=unions)


def multi(level):
    """clusters of two or more rows, and singletons, of one level"""
    sizes = level[2]
    return int((sizes >= 2).sum()), int((sizes == 1).sum())
