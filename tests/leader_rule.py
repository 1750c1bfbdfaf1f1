"""The leader (sphere-exclusion) rule of gsim_db_leader (include/gpusim_hip.h), restated in numpy: the oracle of the GPU tests once
it is fed the pinned per-row scores of oracle_lib (tests/test_leader_host.py checks the restatement itself on a hand-worked table).

The sequential walk takes the rows in ascending order and compares row i with the leaders made so far; here the same walk is done
leader by leader -- when a leader is made, every row still unassigned is compared with it -- which needs one score_row call per
leader.  The two are the same walk: a row is compared with the leaders in the order they were made and leaves at the first that
covers it, and when row p becomes a leader every row below it has been assigned."""
import numpy as np

NONE = 0xFFFFFFFF


def leader_rule(score_row, n, cutoff, seeds=(), max_leaders=None):
    """score_row(r) -> float32 [n]: score(query = row r, row i) for every row i (NaN allowed: never >= cutoff).  Seeds are table
    rows (no row base).  -> (leaders, leader_of, row_score, pairs): the first three as gsim_db_leader returns them (leaders without
    the row base); pairs = the (leader, row) scores the walk evaluates: a row is scored against the leaders in order up to the
    first that covers it."""
    cutoff = np.float32(cutoff)
    cap = n if max_leaders is None else int(max_leaders)
    leader_of = np.full(n, NONE, np.uint32)
    row_score = np.zeros(n, np.float32)
    free = np.ones(n, bool)  # rows without a leader
    leaders = []
    pairs = 0

    def lead(row):
        nonlocal pairs
        pos = len(leaders)
        leaders.append(row)
        leader_of[row] = pos
        row_score[row] = 1.0  # by definition, not by score

    def cover(pos):
        nonlocal pairs
        s = np.asarray(score_row(leaders[pos]), np.float32)
        pairs += int(np.count_nonzero(free))
        with np.errstate(invalid="ignore"):
            got = free & (s >= cutoff)  # a NaN compares false
        leader_of[got] = pos
        row_score[got] = s[got]
        free[got] = False

    for s in seeds:  # leaders even where one covers another
        lead(int(s))
        free[int(s)] = False
    for pos in range(len(leaders)):
        cover(pos)
    at = 0
    while len(leaders) < cap:
        rest = np.flatnonzero(free[at:])
        if rest.size == 0:
            break
        row = at + int(rest[0])
        lead(row)
        free[row] = False
        cover(len(leaders) - 1)
        at = row + 1
    return np.array(leaders, np.uint32), leader_of, row_score, pairs
