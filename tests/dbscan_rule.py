"""The rule of gsim_db_dbscan / gsim_dbscan (include/gpusim_hip.h) restated in numpy: the oracle of tests/test_gpu_dbscan.py and
tests/test_dbscan_host.py.  It never calls the library.

dbscan_rule(S, cutoff, min_pts): S[i, j] = score(query = row i, row j) as float32 (NaN or 0 for 0 / 0: never >= a cutoff in (0, 1]).
The edges are the pairs i < j with S[i, j] >= float32(cutoff) -- the upper triangle, as the device scores a pair once, from its smaller
row -- and an edge's score is S[i, j] of that triangle.  degree = the edges at a row; core = degree + 1 >= min_pts; the clusters are
the components of the cores (components_rule's flood over the core-induced subgraph: numbered in ascending order of their smallest
core row); a non-core row with a core neighbour takes the cluster of its anchor, the core neighbour with the highest score and, among
equal scores, the smallest row; the rest is noise.
Returns (label_of uint32 [n], degree uint32 [n], anchor uint32 [n], first_row uint32 [nc], sizes uint32 [nc], kept = the number of
edges); noise has label_of = anchor = NOISE."""
import numpy as np

from components_rule import components_of_adjacency

NOISE = 0xFFFFFFFF


def dbscan_rule(S, cutoff, min_pts):
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    with np.errstate(invalid="ignore"):
        U = np.triu(S >= np.float32(cutoff), 1)
    A = U | U.T
    score = np.where(U, S, np.float32(0))
    score = score + score.T  # an edge's score, under both of its rows
    degree = A.sum(1).astype(np.uint32)
    core = degree.astype(np.int64) + 1 >= int(min_pts)
    label_of = np.full(n, NOISE, np.uint32)
    anchor = np.full(n, NOISE, np.uint32)
    cores = np.flatnonzero(core)
    sub, first_sub, sizes = components_of_adjacency(A[np.ix_(cores, cores)])
    label_of[cores] = sub
    anchor[cores] = cores
    first_row = cores[first_sub].astype(np.uint32) if len(cores) else np.zeros(0, np.uint32)
    sizes = sizes.astype(np.uint32).copy() if len(cores) else np.zeros(0, np.uint32)
    for x in np.flatnonzero(~core):
        near = np.flatnonzero(A[x] & core)
        if len(near):
            best = near[score[x, near] == score[x, near].max()].min()
            anchor[x] = best
            label_of[x] = label_of[best]
            sizes[label_of[best]] += 1
    return label_of, degree, anchor, first_row, sizes, int(U.sum())


def census(want):
    """(cores, borders, noise, clusters) of a dbscan_rule result"""
    label_of, _, anchor, first_row, _, _ = want
    n = len(label_of)
    cores = int((anchor == np.arange(n)).sum())
    noise = int((label_of == NOISE).sum())
    return cores, n - cores - noise, noise, len(first_row)
