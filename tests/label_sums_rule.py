"""The result rule of gsim_db_label_sums, gsim_label_silhouette and gsim_label_medoids (include/gpusim_hip.h) in numpy and Python
integers.  Scores come from the oracle: S[i, j] = score(query = row i, row j) as one f32 divide, 0 / 0 taken as 0.

    q(s)       = (uint64) floor(f32(s * 2^31))               the product is exact in f32, the conversion truncates
    Q[i, l]    = sum of q(S[i, j]) over j != i with labels[j] == l
    own_q[i]   = Q[i, labels[i]]
    other[i]   = the l != labels[i], sizes[l] > 0, of the greatest Q[i, l] / sizes[l] as an exact fraction, the lowest l among equals
    a, b, sil  = the four double operations of the header, written out below

The argmax: float64 means only pick the labels that can be the maximum (every label whose rounded mean is within 1e-9 relative of
the greatest rounded mean; a double's relative error is 1.2e-16, so the true maximum is among them); between those the comparison is
Q1 * n2 against Q2 * n1 in Python integers, ascending labels, replaced only on strictly greater."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O

NONE = 0xFFFFFFFF
TAN = {}


def score_matrix(db, kw=TAN, nthreads=16):
    """S[i, j] = the oracle's f32 score of row i (the query) against row j; 0 / 0 is 0.0 (as tests/test_gpu_components.py's
    score_matrix, with the NaN of the raw Tanimoto replaced)"""
    db = np.ascontiguousarray(db, dtype=np.uint32)
    n = len(db)
    S = np.zeros((n, n), np.float32)
    if kw.get("metric", O.METRIC_TANIMOTO) == O.METRIC_TANIMOTO:
        def one(r):
            S[r] = O.tanimoto_raw(db[r], db)[0]
    else:
        def one(r):
            hits, _ = O.search(db[r], db, n, 0.0, O.METRIC_TVERSKY, kw["alpha"], kw["beta"])
            S[r, hits["row"]] = hits["score"]
    with ThreadPoolExecutor(nthreads) as pool:
        list(pool.map(one, range(n)))
    np.nan_to_num(S, copy=False, nan=0.0)
    assert float(S.min()) >= 0.0 and float(S.max()) <= 1.0
    return S


def quantise(S):
    """q of every score: f32 product, truncated"""
    p = np.asarray(S, np.float32) * np.float32(2147483648.0)
    assert p.dtype == np.float32
    return np.floor(p).astype(np.uint64)


def inexact(S):
    """pairs whose s * 2^31 is not an integer: truncation acts on them"""
    p = np.asarray(S, np.float32).astype(np.float64) * 2147483648.0
    return p != np.floor(p)


def label_matrix(S, labels, nlabels):
    """-> (Q uint64 [n, number of non-empty labels], those labels ascending, sizes [nlabels]); the rows and columns of
    GSIM_LABEL_NONE rows are left out of the sums, Q's rows of such rows are zero"""
    labels = np.asarray(labels, np.uint32)
    n = len(labels)
    q = quantise(S)
    q[np.arange(n), np.arange(n)] = 0  # j != i
    on = labels != NONE
    sizes = np.bincount(labels[on], minlength=nlabels).astype(np.uint32)
    order = np.flatnonzero(on)[np.argsort(labels[on], kind="stable")]
    present = np.flatnonzero(sizes)
    if len(present) == 0:
        return np.zeros((n, 0), np.uint64), present, sizes
    starts = np.concatenate([[0], np.cumsum(sizes[present], dtype=np.int64)[:-1]]).astype(np.int64)
    Q = np.add.reduceat(q[:, order], starts, axis=1)
    Q[~on] = 0
    return Q, present, sizes


def sums(S, labels, nlabels):
    """-> (own_q uint64, other_label uint32, other_q uint64, sizes uint32, ties: rows whose best mean two labels share)"""
    labels = np.asarray(labels, np.uint32)
    n = len(labels)
    Q, present, sizes = label_matrix(S, labels, nlabels)
    own = np.zeros(n, np.uint64)
    other = np.full(n, NONE, np.uint32)
    other_q = np.zeros(n, np.uint64)
    ties = []
    col_of = {int(l): c for c, l in enumerate(present)}
    psize = sizes[present].astype(np.float64)
    for i in range(n):
        L = int(labels[i])
        if L == NONE:
            continue
        own[i] = Q[i, col_of[L]]
        if len(present) < 2:
            continue
        mean = Q[i].astype(np.float64) / psize
        mean[col_of[L]] = -1.0
        best_l, best_q, best_n, shared = None, 0, 1, False
        for c in np.flatnonzero(mean >= mean.max() * (1.0 - 1e-9)):  # ascending labels
            qc, nc = int(Q[i, c]), int(sizes[present[c]])
            if best_l is None or qc * best_n > best_q * nc:
                best_l, best_q, best_n, shared = int(present[c]), qc, nc, False
            elif qc * best_n == best_q * nc:
                shared = True
        other[i], other_q[i] = best_l, best_q
        if shared:
            ties.append(i)
    return own, other, other_q, sizes, ties


def silhouette(labels, own_q, other_label, other_q, sizes):
    """-> (sil float64 [n], label_mean float64 [nlabels], mean): the operations of the header, one rounding each, sums in
    ascending row order"""
    n, nlabels = len(labels), len(sizes)
    sil = np.zeros(n, np.float64)
    lsum = [0.0] * nlabels
    total, labelled = 0.0, 0
    for i in range(n):
        L = int(labels[i])
        if L == NONE:
            continue
        v = 0.0
        if int(sizes[L]) >= 2 and int(other_label[i]) != NONE:
            a = float(np.float64(np.uint64(own_q[i]))) / float(int(sizes[L]) - 1) * 2.0 ** -31
            b = float(np.float64(np.uint64(other_q[i]))) / float(int(sizes[int(other_label[i])])) * 2.0 ** -31
            d = 1.0 - min(a, b)
            v = (a - b) / d if d > 0 else 0.0
        sil[i] = v
        lsum[L] += v
        total += v
        labelled += 1
    label_mean = np.array([lsum[l] / float(int(sizes[l])) if int(sizes[l]) else 0.0 for l in range(nlabels)], np.float64)
    return sil, label_mean, (total / float(labelled) if labelled else 0.0)


def medoids(labels, own_q, nlabels):
    """-> uint32 [nlabels]: the row of the greatest own_q, the lowest among equals; NONE for an empty label"""
    out = np.full(nlabels, NONE, np.uint32)
    for i in range(len(labels)):
        L = int(labels[i])
        if L != NONE and (out[L] == NONE or int(own_q[i]) > int(own_q[out[L]])):
            out[L] = i
    return out
