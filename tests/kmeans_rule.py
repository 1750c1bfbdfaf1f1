"""The rules of gsim_db_assign, gsim_db_label_counts, gsim_label_centroids and gsim_db_kmeans restated in numpy, on top of the
oracle's scores.  Nothing here calls the library: the tests compare the library with this.

The score matrix comes the way tests/test_gpu_scores.py builds it: oracle_lib.search with k = N at cutoff 0, the centre as the
query (so alpha weighs the centre's bits), scattered by row; a 0 / 0 pair is 0.0."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O

F = np.float32
LABEL_NONE = 0xFFFFFFFF
TAN = dict()


def tv(alpha, beta):
    return dict(metric=O.METRIC_TVERSKY, alpha=alpha, beta=beta)


def score_matrix(centres, db, kw=TAN, nthreads=16):
    """S[c, i] = the oracle's f32 score of centre c (the query) against table row i"""
    centres = np.ascontiguousarray(centres, dtype=np.uint32)
    n = len(db)

    def one(c):
        hits, _ = O.search(centres[c], db, n, 0.0, kw.get("metric", O.METRIC_TANIMOTO), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        assert len(hits) == n
        row = np.empty(n, F)
        row[hits["row"]] = hits["score"]
        return row
    with ThreadPoolExecutor(nthreads) as pool:
        S = np.stack(list(pool.map(one, range(len(centres)))))
    assert not np.isnan(S).any() and float(S.min()) >= 0.0
    S.setflags(write=False)
    return S


def assign(S):
    """-> (label uint32, score float32): the arg-max of the f32 scores down every column, the LOWEST centre among equals"""
    label = np.argmax(S, axis=0)  # (numpy: the first occurrence of the maximum)
    score = S[label, np.arange(S.shape[1])]
    assert (score == S.max(axis=0)).all()
    return label.astype(np.uint32), np.ascontiguousarray(score, dtype=F)


def tied(S):
    """rows whose maximum is attained by two or more centres"""
    return np.flatnonzero((S == S.max(axis=0)).sum(axis=0) >= 2)


def bits(rows):
    """rows x fp_bits 0/1 bytes: bit k is bit k % 32 of word k // 32"""
    rows = np.ascontiguousarray(rows, dtype="<u4")
    return np.unpackbits(rows.view(np.uint8).reshape(len(rows), -1), axis=1, bitorder="little")


def label_counts(db, labels, nlabels):
    """-> (counts uint32 [nlabels, fp_bits], sizes uint32 [nlabels]); LABEL_NONE rows are counted nowhere"""
    labels = np.asarray(labels, dtype=np.uint32)
    assert len(labels) == len(db)
    b = bits(db)
    counts = np.zeros((nlabels, b.shape[1]), np.uint32)
    sizes = np.zeros(nlabels, np.uint32)
    keep = labels != LABEL_NONE
    assert (labels[keep] < nlabels).all()
    np.add.at(sizes, labels[keep], 1)
    order = np.argsort(labels[keep], kind="stable")
    lab, rows = labels[keep][order], b[keep][order]
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]) if len(lab) else np.zeros(0, np.int64)
    if len(lab):
        counts[lab[starts]] = np.add.reduceat(rows.astype(np.uint32), starts, axis=0)
    return counts, sizes


def centroids(counts, sizes, previous=None):
    """bit k of centre l is set iff 2 * counts[l, k] >= sizes[l]; an empty label keeps previous[l] (or zeros)"""
    counts = np.asarray(counts, dtype=np.uint64)
    sizes = np.asarray(sizes, dtype=np.uint64)
    nlabels, fp_bits = counts.shape
    assert (counts <= sizes[:, None]).all()
    on = (2 * counts >= sizes[:, None]).astype(np.uint8)
    out = np.packbits(on, axis=1, bitorder="little").view("<u4").reshape(nlabels, fp_bits // 32).astype(np.uint32)
    empty = sizes == 0
    out[empty] = 0 if previous is None else np.asarray(previous, dtype=np.uint32).reshape(nlabels, -1)[empty]
    return out


def kmeans(db, init, max_iter, kw=TAN):
    """-> dict(centres, label, score, sizes, iterations, converged, history = [(centres_t, label_t)])"""
    assert max_iter >= 1
    m = len(init)
    C = np.ascontiguousarray(init, dtype=np.uint32).copy()
    history, prev, t = [], None, 0
    while True:
        label, score = assign(score_matrix(C, db, kw))
        history.append((C.copy(), label.copy()))
        converged = prev is not None and np.array_equal(label, prev)
        if converged or t + 1 == max_iter:
            break
        counts, sizes = label_counts(db, label, m)
        C = centroids(counts, sizes, C)
        prev = label
        t += 1
    return dict(centres=C, label=label, score=score, sizes=np.bincount(label, minlength=m).astype(np.uint32), iterations=t + 1,
                converged=int(converged), history=history)
