"""The result rule of gsim_db_knn_join / gsim_db_knn_queries (include/gpusim_hip.h), restated in numpy on a rectangular score matrix
(tests/test_knn_join_host.py checks the restatement on a hand-worked table; tests/test_gpu_knn_join.py takes its expected values
from oracle_lib.search, as the rule's first sentence states them).

List i holds the table rows j with S[i, j] >= cutoff -- S[i, j] = score(query = left row i, table row j), taken from the left
row's side; a NaN is never >= anything -- in (score descending, row ascending) order, cut to the first k: a boundary tie group
keeps its lowest rows.  No pair is excluded, unless `exclude_self` says that the left table IS the table (GSIM_KNN_EXCLUDE_SELF):
the pair (left row i, table row i) is then left out.  `row_base` is the TABLE's and is added to the indices; the left side's base plays no part."""
import numpy as np


def knn_join_rule(S, k, cutoff, lrow_begin=0, lrow_end=None, row_base=0, exclude_self=False):
    """S: float32 [nl, n].  -> CSR (indptr uint64 [lrow_end - lrow_begin + 1], indices uint32 (+ row_base), scores float32)."""
    S = np.asarray(S, np.float32)
    lrow_end = S.shape[0] if lrow_end is None else lrow_end
    cutoff = np.float32(cutoff)
    indptr, indices, scores = [0], [], []
    for i in range(lrow_begin, lrow_end):
        with np.errstate(invalid="ignore"):
            ok = S[i] >= cutoff  # a NaN compares false
        if exclude_self:
            ok[i] = False
        rows = np.flatnonzero(ok)
        order = np.lexsort((rows, -S[i, rows].astype(np.float64)))[:k]  # score descending, then row ascending
        indices.append(rows[order] + row_base)
        scores.append(S[i, rows[order]])
        indptr.append(indptr[-1] + len(order))
    return (np.array(indptr, np.uint64), np.concatenate(indices).astype(np.uint32) if indices else np.zeros(0, np.uint32),
            np.concatenate(scores).astype(np.float32) if scores else np.zeros(0, np.float32))
