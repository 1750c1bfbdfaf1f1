"""The result rule of gsim_db_search_labels (include/gpusim_hip.h) in numpy, over the oracle's f32 scores.

    pair_hits   every row's gsim_hit against a query at cutoff 0, in row order: the oracle's score (0 / 0 taken as 0), common, popc_db
    one_query   apply the cutoff (score >= cutoff ? score : 0 in f32), drop the GSIM_LABEL_NONE rows, keep all of the rest when
                cutoff <= 0 and the rows with score != 0 otherwise, group by label, take the lexicographic arg-max on (score, -row),
                count, rank the labels' bests by (score descending, row ascending)
    expect      one_query for every query, stacked the way capi.Table.search_labels returns its arrays

Nothing here is taken from the code under test; the tests compare everything exactly."""
import numpy as np

import oracle_lib as O

NONE = 0xFFFFFFFF
HIT = O.HIT_DTYPE
NO_HIT = np.array([(0xFFFFFFFF, 0.0, 0, 0)], dtype=HIT)[0]


def pair_hits(db, queries, kw=None):
    """-> HIT_DTYPE [nq, N]: entry [q, r] is row r's hit for query q at cutoff 0, `row` = r (no row base)"""
    kw = kw or {}
    db = np.ascontiguousarray(db, dtype=np.uint32)
    queries = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, db.shape[1])
    n = len(db)
    out = np.zeros((len(queries), n), dtype=HIT)
    for q, query in enumerate(queries):
        hits, approx = O.search(query, db, n, 0.0, kw.get("metric", O.METRIC_TANIMOTO), kw.get("alpha", 1.0), kw.get("beta", 1.0), nthreads=8)
        assert len(hits) == n and approx == n and not np.isnan(hits["score"]).any()
        out[q, hits["row"]] = hits
    assert (out["row"] == np.arange(n)[None, :]).all()
    return out


def after_cutoff(score, cutoff):
    """score >= cutoff ? score : 0, compared in f32"""
    score = np.asarray(score, np.float32)
    return np.where(score >= np.float32(cutoff), score, np.float32(0.0)).astype(np.float32)


def one_query(H, labels, nlabels, k, cutoff, row_base=0):
    """H: HIT_DTYPE [N] in row order -> dict(hits, hit_labels, count, approx, rows_kept, label_best [nlabels], label_kept [nlabels])"""
    labels = np.asarray(labels, np.uint32)
    s = after_cutoff(H["score"], cutoff)
    keep = labels != NONE
    if cutoff > 0:
        keep &= s != 0
    idx = np.flatnonzero(keep)
    label_kept = np.bincount(labels[idx], minlength=nlabels).astype(np.uint32)
    order = idx[np.lexsort((idx, -s[idx].astype(np.float64)))]  # the kept rows in (score descending, row ascending) order
    labs, first = np.unique(labels[order], return_index=True)   # a label's best: its first row in that order
    label_best = np.full(nlabels, NO_HIT, dtype=HIT)
    best_rows = order[first]
    rec = H[best_rows].copy()
    rec["score"] = s[best_rows]
    rec["row"] = (best_rows + row_base).astype(np.uint32)
    label_best[labs] = rec
    ranked = order[np.sort(first)]                              # the bests, still in canonical order
    top = ranked[:k]
    return dict(hits=label_best[labels[top]], hit_labels=labels[top].astype(np.uint32), count=len(top), approx=len(labs), rows_kept=len(idx),
                label_best=label_best, label_kept=label_kept)


def expect(H, labels, nlabels, k, cutoff, row_base=0):
    """one_query for every query of H [nq, N], as capi.Table.search_labels(..., per_label=True) lays its arrays out (hits and
    hit_labels zero behind counts[q])"""
    nq = len(H)
    out = dict(hits=np.zeros((nq, max(k, 1)), dtype=HIT), hit_labels=np.zeros((nq, max(k, 1)), np.uint32), counts=np.zeros(nq, np.uint32),
               approx=np.zeros(nq, np.uint64), rows_kept=np.zeros(nq, np.uint64), label_best=np.zeros((nq, nlabels), dtype=HIT),
               label_kept=np.zeros((nq, nlabels), np.uint32))
    for q in range(nq):
        w = one_query(H[q], labels, nlabels, k, cutoff, row_base)
        out["hits"][q, :w["count"]] = w["hits"]
        out["hit_labels"][q, :w["count"]] = w["hit_labels"]
        out["counts"][q] = w["count"]
        out["approx"][q] = w["approx"]
        out["rows_kept"][q] = w["rows_kept"]
        out["label_best"][q] = w["label_best"]
        out["label_kept"][q] = w["label_kept"]
    return out


def same(got, want, what=""):
    """everything exactly: hits and label_best as bytes (the valid entries), labels, counts, approx, rows_kept, label_kept"""
    assert np.array_equal(got["counts"], want["counts"]), (what, "counts", got["counts"], want["counts"])
    assert np.array_equal(got["approx"], want["approx"]), (what, "approx", got["approx"], want["approx"])
    assert np.array_equal(got["rows_kept"], want["rows_kept"]), (what, "rows_kept", got["rows_kept"], want["rows_kept"])
    for q, n in enumerate(want["counts"]):
        assert got["hits"][q, :n].tobytes() == want["hits"][q, :n].tobytes(), (what, "hits of query", q, got["hits"][q, :n][:5], want["hits"][q, :n][:5])
        assert np.array_equal(got["hit_labels"][q, :n], want["hit_labels"][q, :n]), (what, "hit_labels of query", q)
    if "label_best" in got:
        bad = np.flatnonzero((got["label_best"] != want["label_best"]).ravel())
        assert got["label_best"].tobytes() == want["label_best"].tobytes(), (what, "label_best", bad[:5], got["label_best"].ravel()[bad[:5]],
                                                                             want["label_best"].ravel()[bad[:5]])
        assert np.array_equal(got["label_kept"], want["label_kept"]), (what, "label_kept", np.flatnonzero((got["label_kept"] != want["label_kept"]).ravel())[:5])
