"""The MaxMin picking rule of gsim_db_maxmin (include/gpusim_hip.h), restated in numpy: the oracle of the GPU tests once it is
fed the pinned per-row scores of oracle_lib (tests/test_maxmin_host.py checks the restatement itself on hand-built tables)."""
import numpy as np


def maxmin_rule(score_row, n, npicks, seeds=(), max_score=1.0):
    """score_row(r) -> float32 [n]: score(query = row r, row i) for every row i (NaN allowed).  Seeds are table rows (no row
    base).  -> (picks, pick_scores, row_score, nearest) as gsim_db_maxmin returns them, picks without the row base."""
    seeds = [int(s) for s in seeds]
    maxsim = np.full(n, -1.0, np.float32)
    nearest = np.zeros(n, np.uint32)
    picked = np.zeros(n, bool)
    if npicks == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32), maxsim, nearest
    picks = [seeds[0] if seeds else 0]
    pscores = [np.float32(0.0)]
    picked[picks[0]] = True
    j = 0
    while True:
        s = np.asarray(score_row(picks[j]), np.float32)
        s = np.where(np.isnan(s), np.float32(0.0), s)
        upd = (s > maxsim) & ~picked  # only a strictly greater score moves maxsim / nearest
        maxsim[upd] = s[upd]
        nearest[upd] = j
        if len(picks) == npicks:
            break
        if j + 1 < len(seeds):
            r = seeds[j + 1]
            sc = maxsim[r]
        else:
            cand = np.where(picked, np.float32(np.inf), maxsim)
            r = int(np.argmin(cand))  # the first minimum: ties to the lowest row
            sc = cand[r]
            if not (sc <= np.float32(max_score)):
                break
        picks.append(r)
        pscores.append(np.float32(sc))
        picked[r] = True
        j += 1
    picks = np.array(picks, np.uint32)
    row_score = maxsim.copy()
    row_score[picks] = 1.0
    nearest[picks] = np.arange(len(picks), dtype=np.uint32)
    return picks, np.array(pscores, np.float32), row_score, nearest
