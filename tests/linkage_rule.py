"""The rule of gsim_db_linkage / gsim_linkage (include/gpusim_hip.h) in numpy, written twice on a float32 score matrix of which only the
entries i < j are read:

    greedy(S, kind)   the definition: at every step the pair of live clusters (a < b) first in ORDER L = (similarity descending, a
                      ascending, b ascending) is merged -- a cached best partner per row, a global argmax over the rows;
    chain(S, kind)    the nearest-neighbour chain with the library's restart and tie rules (the chain starts at the lowest live slot;
                      the nearest neighbour of the tip X is the live Y of the greatest similarity, the lowest Y among equals; when it
                      is the element below the tip the two are merged into the lower slot), then the replay of the executed merges
                      into greedy order.  It also returns the scans and the deepest the chain got.

Both keep one int64 matrix M: the bits of the f32 scores for complete linkage (non-negative floats order as their bits do), merged by
minimum; q(s) = floor(f32(s * 2^31)) for average linkage, merged by addition.  A similarity is the exact fraction M / den with den = 1
(complete) or |A| |B| (average); fractions are compared exactly in int64 by quotient and remainder (frac_cmp), which needs
denominators below 2^31.  Both take optional initial cluster sizes and, for average linkage, initial pair sums.
"""
import heapq
from fractions import Fraction

import numpy as np

COMPLETE, AVERAGE = 0, 1
MERGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("left", np.uint32), ("right", np.uint32), ("size", np.uint32),
                        ("score", np.float32), ("sum_q", np.uint64)])


def q(S):
    """q(s) = floor(f32(s * 2^31)): the product is exact in f32, the conversion truncates"""
    return np.floor(np.asarray(S, np.float32) * np.float32(2147483648.0)).astype(np.int64)


def frac_cmp(x, p, y, r):
    """sign of x / p - y / r, exact: x, y >= 0 int64, 0 < p, r < 2^31"""
    x, p, y, r = (np.asarray(v, np.int64) for v in (x, p, y, r))
    qx, qy = x // p, y // r
    rx, ry = x - qx * p, y - qy * r
    return np.where(qx != qy, np.sign(qx - qy), np.sign(rx * r - ry * p))


def best_fraction(x, p):
    """the positions of the greatest x / p, ascending"""
    assert int(p.max()) < 2**31 and int(p.min()) > 0
    k = int(np.argmax(x.astype(np.float64) / p))
    while True:
        d = frac_cmp(x, p, x[k], p[k])
        better = np.flatnonzero(d > 0)
        if len(better) == 0:
            return np.flatnonzero(d == 0)
        k = int(better[0])


def _matrix(S, kind, sums):
    S = np.ascontiguousarray(S, np.float32)
    n = S.shape[0]
    assert S.shape == (n, n)
    if sums is not None:
        up = np.asarray(sums, np.int64)
    elif kind == AVERAGE:
        up = q(S)
    else:
        up = (S + np.float32(0.0)).view(np.uint32).astype(np.int64)
    M = np.triu(up, 1)
    return M + M.T, n


def _record(a, b, ida, idb, sa, sb, v, kind):
    m = np.zeros((), MERGE_DTYPE)
    m["a"], m["b"], m["left"], m["right"], m["size"] = a, b, ida, idb, sa + sb
    if kind == AVERAGE:
        m["sum_q"] = v
        m["score"] = np.float32((float(int(v)) / float(int(sa) * int(sb))) * 2.0**-31)
    else:
        m["score"] = np.array([v], np.uint32).view(np.float32)[0]
        m["sum_q"] = q(m["score"])
    return m


def greedy(S, kind, sizes=None, sums=None):
    M, n = _matrix(S, kind, sums)
    size = np.ones(n, np.int64) if sizes is None else np.asarray(sizes, np.int64).copy()
    den = (lambda: size) if kind == AVERAGE else (lambda: np.ones(n, np.int64))
    live = np.ones(n, bool)
    ids = np.arange(n)
    best_b = np.full(n, -1)  # of every live row a: the live b > a first in (similarity descending, b ascending)

    def row_best(a):
        cand = a + 1 + np.flatnonzero(live[a + 1:])
        if len(cand) == 0:
            return -1
        return int(cand[best_fraction(M[a, cand], den()[cand])[0]])

    for a in range(n):
        best_b[a] = row_best(a)
    out = np.zeros(max(n - 1, 0), MERGE_DTYPE)
    for m in range(n - 1):
        rows = np.flatnonzero(live & (best_b >= 0))
        d = den()
        top = rows[best_fraction(M[rows, best_b[rows]], d[rows] * d[best_b[rows]])]
        a = int(top[0])
        b = int(best_b[a])
        out[m] = _record(a, b, ids[a], ids[b], size[a], size[b], M[a, b], kind)
        z = np.flatnonzero(live)
        z = z[(z != a) & (z != b)]
        M[a, z] = M[a, z] + M[b, z] if kind == AVERAGE else np.minimum(M[a, z], M[b, z])
        M[z, a] = M[a, z]
        size[a] += size[b]
        size[b] = 0
        live[b] = False
        ids[a] = n + m
        # the rows whose cached partner was a or b, row a itself, and the rows below a for which the new (z, a) comes first
        redo = set(np.flatnonzero(live & ((best_b == a) | (best_b == b))).tolist()) | {a}
        low = np.flatnonzero(live[:a] & (best_b[:a] >= 0))
        low = low[~np.isin(low, list(redo))]
        if len(low):
            d = den()
            c = frac_cmp(M[low, a], np.full(len(low), d[a]), M[low, best_b[low]], d[best_b[low]])
            best_b[low[(c > 0) | ((c == 0) & (a < best_b[low]))]] = a
        for r in redo:
            best_b[r] = row_best(r)
    return out


def chain(S, kind, sizes=None, sums=None):
    """-> (merges, scans, chain_max)"""
    M, n = _matrix(S, kind, sums)
    size = np.ones(n, np.int64) if sizes is None else np.asarray(sizes, np.int64).copy()
    size0 = size.copy()
    live = np.ones(n, bool)
    stack, raw, scans, chain_max = [], [], 0, 0
    while len(raw) < n - 1:
        if not stack:
            stack.append(int(np.flatnonzero(live)[0]))
            chain_max = max(chain_max, 1)
        x = stack[-1]
        cand = np.flatnonzero(live)
        cand = cand[cand != x]
        y = int(cand[best_fraction(M[x, cand], size[cand] if kind == AVERAGE else np.ones(len(cand), np.int64))[0]])
        scans += 1
        if len(stack) >= 2 and stack[-2] == y:
            a, b = min(x, y), max(x, y)
            raw.append((a, b, int(size[a]), int(size[b]), int(M[a, b])))
            z = cand[cand != y]
            M[a, z] = M[a, z] + M[b, z] if kind == AVERAGE else np.minimum(M[a, z], M[b, z])
            M[z, a] = M[a, z]
            size[a] += size[b]
            size[b] = 0
            live[b] = False
            del stack[-2:]
        else:
            stack.append(y)
            chain_max = max(chain_max, len(stack))
    # the replay: among the executed merges whose two clusters exist, the one first in L
    last, nxt, waits = {}, {}, [0] * len(raw)
    for r, (a, b, _, _, _) in enumerate(raw):
        for slot in (a, b):
            if slot in last:
                nxt[last[slot]] = r
                waits[r] += 1
        last[a] = r
        last.pop(b, None)

    def key(r):
        a, b, sa, sb, v = raw[r]
        return (-Fraction(v, sa * sb if kind == AVERAGE else 1), a, b, r)

    heap = [key(r) for r in range(len(raw)) if waits[r] == 0]
    heapq.heapify(heap)
    ids = list(range(n))
    out = np.zeros(max(n - 1, 0), MERGE_DTYPE)
    m = 0
    while heap:
        r = heapq.heappop(heap)[3]
        a, b, sa, sb, v = raw[r]
        out[m] = _record(a, b, ids[a], ids[b], sa, sb, v, kind)
        ids[a] = n + m
        m += 1
        if r in nxt:
            waits[nxt[r]] -= 1
            if waits[nxt[r]] == 0:
                heapq.heappush(heap, key(nxt[r]))
    assert m == len(raw) and int(size0.sum()) == int(size.sum())
    return out, scans, chain_max


def cut(merges, n, t):
    """The flat clusters at t straight from the dendrogram: scores never increase, so they are what the merges with score >= t leave --
    walked through left / right.  -> (component_of, first_row, sizes), components numbered by their smallest row ascending."""
    k = int(np.count_nonzero(merges["score"] >= np.float32(t)))
    assert (merges["score"][:k] >= np.float32(t)).all()
    leaves = {i: [i] for i in range(n)}
    for m in range(k):
        leaves[n + m] = leaves.pop(int(merges["left"][m])) + leaves.pop(int(merges["right"][m]))
    comps = sorted((min(v), v) for v in leaves.values())
    component_of = np.zeros(n, np.uint32)
    for c, (_, rows) in enumerate(comps):
        component_of[rows] = c
    return component_of, np.array([f for f, _ in comps], np.uint32), np.array([len(r) for _, r in comps], np.uint32)
