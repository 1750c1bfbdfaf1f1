"""The rule of gsim_db_components / gsim_components (include/gpusim_hip.h) restated in numpy: the oracle of
tests/test_gpu_components.py and tests/test_components_host.py.

components_rule(S, cutoff): S[i, j] = score(query = row i, row j) as float32 (NaN or 0 for 0 / 0: never >= a cutoff in (0, 1]).  The
edges are the pairs i < j with S[i, j] >= float32(cutoff) -- the upper triangle, as the device scores a pair once, from its smaller
row.  Components are found by flooding from every row not yet reached, in ascending order, so they come numbered in ascending order
of their smallest row.  Returns (component_of uint32 [n], first_row uint32 [nc], sizes uint32 [nc], kept = the number of edges)."""
import numpy as np


def components_of_adjacency(A):
    """A: symmetric boolean n x n (the diagonal is ignored)."""
    n = A.shape[0]
    component_of = np.full(n, 0xFFFFFFFF, np.uint32)
    first_row, sizes = [], []
    for r in range(n):
        if component_of[r] != 0xFFFFFFFF:
            continue
        member = np.zeros(n, bool)
        member[r] = True
        frontier = member.copy()
        while frontier.any():
            reached = A[frontier].any(0) & ~member
            member |= reached
            frontier = reached
        assert not (component_of[member] != 0xFFFFFFFF).any() and int(np.flatnonzero(member)[0]) == r
        component_of[member] = len(first_row)
        first_row.append(r)
        sizes.append(int(member.sum()))
    return component_of, np.array(first_row, np.uint32), np.array(sizes, np.uint32)


def components_rule(S, cutoff):
    S = np.asarray(S, np.float32)
    with np.errstate(invalid="ignore"):
        U = np.triu(S >= np.float32(cutoff), 1)
    return components_of_adjacency(U | U.T) + (int(U.sum()),)


def csr_of(A):
    """CSR (indptr uint64, indices uint32) of a boolean matrix, columns ascending."""
    indptr = np.zeros(A.shape[0] + 1, np.uint64)
    indptr[1:] = np.cumsum(A.sum(1))
    return indptr, np.nonzero(A)[1].astype(np.uint32)


def refines(fine, coarse):
    """every component of `fine` lies inside one component of `coarse`"""
    seen = {}
    return all(seen.setdefault(int(f), int(c)) == int(c) for f, c in zip(fine, coarse))
