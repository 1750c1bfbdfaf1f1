"""The rule of gsim_db_core_scores / gsim_db_mreach_mst / gsim_db_hdbscan and of their host companions gsim_mreach_mst and
gsim_mst_hdbscan (include/gpusim_hip.h) restated in Python: the oracle of tests/test_gpu_hdbscan.py and tests/test_hdbscan_host.py.

S[i, j] = score(row i, row j) as float32, symmetric (NaN or 0 for 0 / 0, 0 for a pair a graph does not list: never >= a cutoff > 0).

core_scores(S, cutoff, min_pts): the (min_pts - 1)-th largest of row i's scores >= cutoff to OTHER rows, 0 where there are fewer, 1 for
min_pts == 1.
mreach_matrix(S, cutoff, min_pts) -> (M, core): M[i, j] = min(S[i, j], core[i], core[j]) where S[i, j] >= cutoff and that minimum is
>= cutoff, else 0.
mreach_rule(S, cutoff, min_pts) -> (edges, core): mst_rule.kruskal on M -- the forest in order E = (m descending, a, b).

condensed_tree(edges, n): the multiway dendrogram.  Equal scores are one event: for each distinct score s, descending, the components of
{edges with score >= s} that contain an edge of score s are the nodes at s; a node's children are the components of {edges > s} inside
it, nodes or single rows.
hdbscan_rule(edges, n, floor, min_cluster_size, flags): the clusters, their stabilities as fractions.Fraction (exact), the selection
(EOM or LEAF, with or without NO_ROOTS), the labels -- and, for EOM, the relative margin |stability - sub| / max(stability, sub) of
every comparison made, so that a test can say that no comparison hangs on the rounding of a double."""
from fractions import Fraction

import numpy as np

from mst_rule import EDGE, mst_rule

NOISE = 0xFFFFFFFF
EOM, LEAF, NO_ROOTS = 0, 1, 2


def core_scores(S, cutoff, min_pts):
    S = np.asarray(S, np.float32)
    n = len(S)
    if min_pts == 1:
        return np.ones(n, np.float32)
    with np.errstate(invalid="ignore"):
        ok = S >= np.float32(cutoff)
    np.fill_diagonal(ok, False)
    k = min_pts - 1
    core = np.zeros(n, np.float32)
    for i in range(n):
        mine = np.sort(S[i, ok[i]])[::-1]
        if len(mine) >= k:
            core[i] = mine[k - 1]
    return core


def mreach_matrix(S, cutoff, min_pts):
    S = np.asarray(S, np.float32)
    core = core_scores(S, cutoff, min_pts)
    with np.errstate(invalid="ignore"):
        ok = S >= np.float32(cutoff)
    np.fill_diagonal(ok, False)
    M = np.where(ok, np.minimum(np.where(ok, S, 0), np.minimum(core[:, None], core[None, :])), 0).astype(np.float32)
    if min_pts == 1:  # nothing is capped, whatever the scores are
        M = np.where(ok, S, 0).astype(np.float32)
    M[M < np.float32(cutoff)] = 0
    return M, core


def mreach_rule(S, cutoff, min_pts):
    M, core = mreach_matrix(S, cutoff, min_pts)
    return mst_rule(M, cutoff), core


def tied(edges):
    _, counts = np.unique(edges["score"], return_counts=True)
    return int(counts[counts > 1].sum())


class Node:
    def __init__(self, level, children):
        self.level = level          # float32 value as a Python float
        self.children = children    # Node, or int: a single row
        self.rows = sorted(r for c in children for r in (c.rows if isinstance(c, Node) else [c]))


def size(child):
    return len(child.rows) if isinstance(child, Node) else 1


def rows_of(child):
    return child.rows if isinstance(child, Node) else [child]


def condensed_tree(edges, n):
    """-> the top of every tree of the forest: a Node, or an int for a row no edge touches"""
    top = {r: r for r in range(n)}  # component key -> Node or row
    key_of = list(range(n))         # row -> component key
    scores = edges["score"]
    for s in sorted(set(scores.tolist()), reverse=True):
        group = edges[scores == np.float32(s)]
        link = {}

        def root(x):
            while link.get(x, x) != x:
                x = link[x]
            return x

        for a, b in zip(group["a"].tolist(), group["b"].tolist()):
            x, y = root(key_of[a]), root(key_of[b])
            assert x != y, "a forest has no cycle"
            link[max(x, y)] = min(x, y)
        merged = {}
        for k in {key_of[a] for a in group["a"].tolist()} | {key_of[b] for b in group["b"].tolist()}:
            merged.setdefault(root(k), []).append(k)
        for k, parts in merged.items():
            node = Node(float(s), [top.pop(p) for p in sorted(parts)])
            top[k] = node
            for r in node.rows:
                key_of[r] = k
    return [top[k] for k in sorted(top)]


def hdbscan_rule(edges, n, floor, mcs, flags=EOM):
    """-> dict: label [n], leave float32 [n], first_row, sizes, birth (float32), stability (Fraction) per selected cluster, in their
    numbering; margins: of every EOM comparison; all_stability: of every cluster of the condensed tree"""
    floor = float(np.float32(floor))
    clusters = []  # [parent, node, birth, stability, children, rows at birth]
    last = [None] * n
    leave = np.zeros(n, np.float32)
    work = []

    def born(parent, node, birth):
        clusters.append(dict(parent=parent, node=node, birth=birth, stability=Fraction(0), children=[], rows=list(node.rows)))
        if parent is not None:
            clusters[parent]["children"].append(len(clusters) - 1)
        work.append(len(clusters) - 1)

    for t in condensed_tree(edges, n):
        if size(t) >= mcs:
            born(None, t, floor)
    while work:
        c = work.pop()
        C = clusters[c]
        node, birth = C["node"], Fraction(C["birth"])
        while True:
            s = node.level
            large = [ch for ch in node.children if size(ch) >= mcs]
            for ch in node.children:
                if size(ch) < mcs:
                    for r in rows_of(ch):
                        last[r], leave[r] = c, s
                        C["stability"] += Fraction(s) - birth
            if not large:
                break
            if len(large) == 1:
                node = large[0]
                continue
            for ch in large:
                C["stability"] += len(ch.rows) * (Fraction(s) - birth)
                born(c, ch, s)
            break
    # the selection, bottom-up: children were born after their parents
    selected, shat, margins = set(), {}, []

    def below(c):
        out = []
        for ch in clusters[c]["children"]:
            out += [ch] + below(ch)
        return out

    for c in reversed(range(len(clusters))):
        C = clusters[c]
        if not C["children"]:
            selected.add(c)
            shat[c] = C["stability"]
            continue
        sub = sum(shat[ch] for ch in C["children"])
        if flags & LEAF:
            shat[c] = sub
            continue
        if flags & NO_ROOTS and C["parent"] is None:
            shat[c] = sub
            continue
        big = max(C["stability"], sub)
        margins.append(float(abs(C["stability"] - sub) / big) if big else 0.0)
        if C["stability"] >= sub:
            selected.add(c)
            selected.difference_update(below(c))
            shat[c] = C["stability"]
        else:
            shat[c] = sub
    order = sorted(selected, key=lambda c: clusters[c]["rows"][0])
    number = {c: k for k, c in enumerate(order)}
    label = np.full(n, NOISE, np.uint32)
    for r in range(n):
        c = last[r]
        while c is not None and c not in number:
            c = clusters[c]["parent"]
        if c is not None:
            label[r] = number[c]
    return dict(label=label, leave=leave, first_row=np.array([clusters[c]["rows"][0] for c in order], np.uint32),
                sizes=np.array([len(clusters[c]["rows"]) for c in order], np.uint32),
                birth=np.array([clusters[c]["birth"] for c in order], np.float32), stability=[clusters[c]["stability"] for c in order],
                margins=margins, all_stability=[C["stability"] for C in clusters])


__all__ = ["EDGE", "EOM", "LEAF", "NO_ROOTS", "NOISE", "condensed_tree", "core_scores", "hdbscan_rule", "mreach_matrix", "mreach_rule", "tied"]
