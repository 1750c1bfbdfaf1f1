"""The rule of gsim_db_mst / gsim_mst (include/gpusim_hip.h) restated in Python: the oracle of tests/test_gpu_mst.py and
tests/test_mst_host.py.

mst_rule(S, cutoff): S[i, j] = score(row i, row j) as float32 (NaN or 0 for 0 / 0: never >= a cutoff in (0, 1]).  The edges are the
pairs a < b with S[a, b] >= float32(cutoff) in order E = (score descending, a ascending, b ascending); Kruskal takes them in that order
and keeps an edge iff its ends are not yet connected.  Returns the kept edges, in order E, as capi.MST_EDGE_DTYPE.

boruvka(S, cutoff): the same forest by rounds -- every component takes its E-first outgoing edge -- with the bookkeeping of the device's
owner list: a row scans again only when the partner it holds has joined its own component.  Returns (edges in order E, rounds that
added edges, the owner count of every scan made: one per round, and a last one that finds nothing unless the forest is one tree)."""
import numpy as np

EDGE = np.dtype([("a", np.uint32), ("b", np.uint32), ("score", np.float32)])


def kruskal(a, b, score, n):
    """edges (a < b) of any order -> the forest in order E"""
    order = np.lexsort((b, a, -score.astype(np.float64)))
    parent = list(range(n))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kept = []
    for e in order:
        x, y = root(int(a[e])), root(int(b[e]))
        if x != y:
            parent[max(x, y)] = min(x, y)
            kept.append(e)
            if len(kept) == n - 1:
                break
    out = np.empty(len(kept), EDGE)
    out["a"], out["b"], out["score"] = a[kept], b[kept], score[kept]
    return out


def mst_rule(S, cutoff):
    S = np.asarray(S, np.float32)
    with np.errstate(invalid="ignore"):
        a, b = np.nonzero(np.triu(S >= np.float32(cutoff), 1))
    return kruskal(a.astype(np.uint32), b.astype(np.uint32), S[a, b], len(S))


def boruvka(S, cutoff):
    S = np.asarray(S, np.float32)
    n = len(S)
    with np.errstate(invalid="ignore"):
        ok = S >= np.float32(cutoff)
    np.fill_diagonal(ok, False)
    comp = np.arange(n)
    partner = np.full(n, -1)
    owners = np.ones(n, bool)
    taken, rounds, scans = set(), 0, []
    while True:
        scans.append(int(owners.sum()))
        for i in np.flatnonzero(owners):  # the row's E-first foreign edge: the best score, then the smallest partner
            s = np.where(ok[i] & (comp != comp[i]), S[i], np.float32(-1))
            j = int(np.argmax(s))
            partner[i] = j if s[j] >= 0 else -1
        picks = {}
        for i in np.flatnonzero(partner >= 0):  # the component's E-first held edge
            j = int(partner[i])
            key = (-float(S[i, j]), min(i, j), max(i, j))
            picks[comp[i]] = min(picks.get(comp[i], key), key)
        new = set(picks.values()) - taken
        if not new:
            break
        rounds += 1
        taken |= new
        for _, x, y in new:
            cx, cy = comp[x], comp[y]
            if cx != cy:
                comp[comp == max(cx, cy)] = min(cx, cy)
        held = partner >= 0
        owners = held & (comp[np.where(held, partner, 0)] == comp)
        if len(taken) == n - 1:
            break
    out = np.array(sorted((x, y, -s) for s, x, y in taken), EDGE) if taken else np.empty(0, EDGE)
    out = out[np.lexsort((out["b"], out["a"], -out["score"].astype(np.float64)))]
    return out, rounds, scans
