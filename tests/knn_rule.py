"""The result rule of gsim_db_knn (include/gpusim_hip.h), restated in numpy on a score matrix (tests/test_knn_host.py checks the
restatement on a hand-worked table; tests/test_gpu_knn.py takes its expected values from oracle_lib.search, as the rule's first
sentence states them, and uses this only where a whole score matrix is at hand).

List i holds the rows j != i with S[i, j] >= cutoff -- S[i, j] = score(query = row i, row j), taken from row i's side; a NaN is
never >= anything -- in (score descending, row ascending) order, cut to the first k: a boundary tie group keeps its lowest rows."""
import numpy as np


def knn_rule(S, k, cutoff, row_begin=0, row_end=None, row_base=0):
    """S: float32 [n, n].  -> CSR (indptr uint64 [row_end - row_begin + 1], indices uint32 (+ row_base), scores float32)."""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    row_end = n if row_end is None else row_end
    cutoff = np.float32(cutoff)
    indptr, indices, scores = [0], [], []
    for i in range(row_begin, row_end):
        with np.errstate(invalid="ignore"):
            ok = S[i] >= cutoff  # a NaN compares false
        ok[i] = False
        rows = np.flatnonzero(ok)
        order = np.lexsort((rows, -S[i, rows].astype(np.float64)))[:k]  # score descending, then row ascending
        indices.append(rows[order] + row_base)
        scores.append(S[i, rows[order]])
        indptr.append(indptr[-1] + len(order))
    return (np.array(indptr, np.uint64), np.concatenate(indices).astype(np.uint32) if indices else np.zeros(0, np.uint32),
            np.concatenate(scores).astype(np.float32) if scores else np.zeros(0, np.float32))
