"""The rule of gsim_popindex_* and gsim_db_search_bounded (include/gpusim_hip.h) restated in numpy: the oracle of
tests/test_popindex_host.py and tests/test_gpu_popindex.py.

  order, first   np.lexsort((rows, popc)) and the cumulative bincount
  ub             the enumeration over c with the oracle's score arithmetic: `score` below is gso_score_one in numpy float32 (one
                 rounding per operation, in its order), vectorised because a table of 4096-bit rows has 16 M (b, c) pairs;
                 test_popindex_host.py checks it against oracle_lib's gso_score_one bit for bit
  execution      the cutoff window, stage 1's hull, the stage-2 decision given stage 1's result (the oracle's search over the hull's
                 rows), the route of every scan -- and from them the stats the call has to report
"""
import numpy as np

import oracle_lib as O

TAN, TV = O.METRIC_TANIMOTO, O.METRIC_TVERSKY
F32 = np.float32
GATHER_PERMILLE = 250  # GSIM_SUBSET_GATHER_MAX_PERMILLE's default


def popcounts(db):
    db = np.ascontiguousarray(db, dtype=np.uint32)
    return np.unpackbits(db.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


def order_first(db, base=0):
    """-> (popc, order uint32 with the row base, first uint64 [fp_bits + 2])"""
    popc = popcounts(db)
    rows = np.arange(len(db), dtype=np.int64)
    order = np.lexsort((rows, popc))
    F = db.shape[1] * 32
    first = np.concatenate([[0], np.cumsum(np.bincount(popc, minlength=F + 1))]).astype(np.uint64)
    return popc, (order + base).astype(np.uint32), first


def score(metric, alpha, beta, a, b, c):
    """gso_score_one on arrays: float32, one rounding per operation"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(c, np.int64))
    cf = c.astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == TV:
            t1 = F32(alpha) * (a - c).astype(F32)
            t2 = F32(beta) * (b - c).astype(F32)
            return (cf / ((t1 + t2) + cf)).astype(F32)
        return (cf / (a + b - c).astype(F32)).astype(F32)


def bounds(fp_bits, a, metric=TAN, alpha=1.0, beta=1.0):
    """ub[b], b = 0 .. fp_bits: the largest score over c in [max(0, a + b - fp_bits), min(a, b)], NaN taken as 0"""
    ub = np.empty(fp_bits + 1, F32)
    c = np.arange(0, a + 1, dtype=np.int64)[None, :]
    for b0 in range(0, fp_bits + 1, 512):
        b = np.arange(b0, min(b0 + 512, fp_bits + 1), dtype=np.int64)[:, None]
        s = score(metric, alpha, beta, a, b, c)
        s = np.where(np.isnan(s), F32(0), s)
        valid = (c >= np.maximum(0, a + b - fp_bits)) & (c <= np.minimum(a, b))
        ub[b0:b0 + len(b)] = np.where(valid, s, F32(-np.inf)).max(axis=1)
    return ub


def unit_scores(metric, alpha, beta):
    if metric != TV:
        return True
    return bool(np.isfinite(alpha) and np.isfinite(beta) and alpha >= 0 and beta >= 0 and float(F32(alpha)) + float(F32(beta)) >= 1.0)


def hull_at_least(ub, hull, t):
    """the hull (b0, b1) of the buckets of `hull` whose bound is at least t, or None"""
    if hull is None:
        return None
    b = np.arange(hull[0], hull[1] + 1)
    b = b[ub[hull[0]:hull[1] + 1] >= F32(t)]
    return (int(b[0]), int(b[-1])) if len(b) else None


def rows_of(first, hull):
    return 0 if hull is None else int(first[hull[1] + 1]) - int(first[hull[0]])


def stage1_hull(ub, window, first, target):
    b = np.arange(window[0], window[1] + 1)
    b = b[np.argsort(-ub[window[0]:window[1] + 1].astype(np.float64), kind="stable")]  # ub descending, ties to the lower b
    lo = hi = int(b[0])
    for x in b:
        lo, hi = min(lo, int(x)), max(hi, int(x))
        if rows_of(first, (lo, hi)) >= target:
            break
    return lo, hi


def route(n, N, W, copy, permille=GATHER_PERMILLE):
    """'stream' | 'gather' | 'plain' for a scan of n rows (permille: the GSIM_SUBSET_GATHER_MAX_PERMILLE the handle was created under)"""
    if copy:
        return "stream" if 4 * n <= 3 * N else "plain"
    if permille <= 0 or permille >= 1000:
        return "gather" if permille else "plain"
    row_bytes = W * 4
    return "gather" if n * max(row_bytes, 128) * 1000 <= permille * N * row_bytes else "plain"


def hull_rows(popc, hull):
    """the table rows (ascending) whose popcount lies in the hull"""
    return np.flatnonzero((popc >= hull[0]) & (popc <= hull[1]))


def search_rows(q, db, rows, k, cutoff, kw):
    """the oracle's search over the given rows (ascending) only, rows mapped back"""
    if len(rows) == 0 or k == 0:
        return np.zeros(0, O.HIT_DTYPE)
    hits, _ = O.search(q, db[rows], k, cutoff, kw.get("metric", TAN), kw.get("alpha", 1.0), kw.get("beta", 1.0), nthreads=8)
    hits["row"] = rows[hits["row"]].astype(np.uint32)
    return hits


_bounds_cache = {}


def bounds_cached(fp_bits, a, metric, alpha, beta):
    key = (fp_bits, a, metric, float(alpha), float(beta))
    if key not in _bounds_cache:
        _bounds_cache[key] = bounds(fp_bits, a, metric, alpha, beta)
    return _bounds_cache[key]


def execute(q, db, popc, first, k, cutoff, kw, copy, approx_wanted=True, permille=GATHER_PERMILLE):
    """How the call has to answer one query -> dict(rows_scanned, rows_window, stage: 'one' | 'two' | 'plain', scans: [(route, hull)])"""
    N, W = db.shape
    F = W * 32
    metric, alpha, beta = kw.get("metric", TAN), kw.get("alpha", 1.0), kw.get("beta", 1.0)
    a = int(popcounts(np.asarray(q, np.uint32).reshape(1, -1))[0])
    ub = bounds_cached(F, a, metric, alpha, beta)
    k = min(k, N)
    window = hull_at_least(ub, (0, F), cutoff) if cutoff > 0 else (0, F)
    out = dict(rows_scanned=0, rows_window=rows_of(first, window), scans=[], ub=ub, window=window)
    if rows_of(first, window) == 0:
        out["stage"] = "one"
        return out
    target = max(4 * k, 4096)
    narrow = k >= 1 and (cutoff <= 0 or not approx_wanted) and unit_scores(metric, alpha, beta) and rows_of(first, window) > target
    h1 = stage1_hull(ub, window, first, target) if narrow else window

    def scan(hull):
        r = route(rows_of(first, hull), N, W, copy, permille)
        out["scans"].append((r, hull))
        out["rows_scanned"] += N if r == "plain" else rows_of(first, hull)
        return r

    if scan(h1) == "plain":
        out["stage"] = "plain"
        return out
    done = h1 == window
    if not done:
        hits = search_rows(q, db, hull_rows(popc, h1), k, cutoff, kw)
        if len(hits) == k:
            sk = hits["score"][-1]
            outside = np.r_[ub[window[0]:h1[0]], ub[h1[1] + 1:window[1] + 1]]
            done = bool((outside < sk).all())
            h2 = hull_at_least(ub, window, sk)
        else:
            h2 = window
    if done:
        out["stage"] = "one"
        return out
    out["stage"] = "plain" if scan(h2) == "plain" else "two"
    return out


def expected_stats(plans):
    st = dict(rows_scanned=0, rows_window=0, queries_one_stage=0, queries_two_stage=0, queries_plain=0)
    for p in plans:
        st["rows_scanned"] += p["rows_scanned"]
        st["rows_window"] += p["rows_window"]
        st[{"one": "queries_one_stage", "two": "queries_two_stage", "plain": "queries_plain"}[p["stage"]]] += 1
    return st
