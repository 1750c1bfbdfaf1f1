"""CPU checks of gsim_db_maxmin: argument validation without a GPU (errors, never a CPU fallback), and the numpy restatement of
the picking rule (maxmin_rule.py, the oracle of tests/test_gpu_maxmin.py) on hand-built score tables whose answers are worked
out here."""
import ctypes as C

import numpy as np
import pytest

from gpusimilarity_amd import capi
from maxmin_rule import maxmin_rule

F = np.float32


def sym(n, upper):
    """Symmetric score table, 1.0 on the diagonal, upper[(i, j)] above it."""
    m = np.eye(n, dtype=np.float32)
    for (i, j), v in upper.items():
        m[i, j] = m[j, i] = F(v)
    return m


def rule(m, npicks, seeds=(), max_score=1.0):
    return maxmin_rule(lambda r: m[r], m.shape[0], npicks, seeds, max_score)


def test_ties_go_to_the_lowest_row():
    m = sym(4, {(0, 1): .5, (0, 2): .2, (0, 3): .2, (1, 2): .3, (1, 3): .3, (2, 3): .9})
    # pass 0: maxsim = [-, .5, .2, .2] -> rows 2 and 3 tie at .2: row 2; pass 1 raises row 3 to .9 -> row 1 (.5), then row 3
    picks, ps, rs, nr = rule(m, 4)
    assert picks.tolist() == [0, 2, 1, 3]
    assert ps.tolist() == [F(0), F(.2), F(.5), F(.9)]
    assert rs.tolist() == [1.0] * 4 and nr.tolist() == [0, 2, 1, 3]
    picks, ps, rs, nr = rule(m, 3)
    assert picks.tolist() == [0, 2, 1]
    assert rs.tolist() == [1.0, 1.0, 1.0, F(.9)] and nr.tolist() == [0, 2, 1, 1]


def test_nan_counts_as_zero_and_nearest_ties_go_to_the_earliest_pick():
    nan = float("nan")
    # rows 0 and 1 all-zero (0/0 against each other and themselves), row 2 unlike both
    m = np.array([[nan, nan, 0], [nan, nan, 0], [0, 0, 1]], np.float32)
    picks, ps, rs, nr = rule(m, 2)
    # pass 0: rows 1 and 2 at 0.0 (NaN -> 0) -> row 1; pass 1 scores row 2 at 0.0 again: not greater, nearest stays pick 0
    assert picks.tolist() == [0, 1] and ps.tolist() == [0.0, 0.0]
    assert rs.tolist() == [1.0, 1.0, 0.0] and nr.tolist() == [0, 1, 0]
    picks, ps, _, _ = rule(m, 3)
    assert picks.tolist() == [0, 1, 2] and ps.tolist() == [0.0, 0.0, 0.0]
    m = sym(4, {(0, 1): .1, (0, 2): .2, (0, 3): .4, (1, 2): .3, (1, 3): .4, (2, 3): .1})
    _, _, rs, nr = rule(m, 2)  # row 3 scores .4 against picks 0 and 1: the earliest keeps it
    assert nr[3] == 0 and rs[3] == F(.4) and nr[2] == 1 and rs[2] == F(.3)


M5 = sym(5, {(0, 1): .1, (0, 2): .6, (0, 3): .3, (0, 4): .2, (1, 2): .2, (1, 3): .7, (1, 4): .4, (2, 3): .5, (2, 4): .8,
             (3, 4): .3})


def test_seeds_and_the_max_score_stop():
    # seeds 3, 1: pick 1 scores .7 against pick 0 (seeds are picked whatever their score); then rows 0 (.3), 4 (.4), 2 (.8)
    picks, ps, rs, nr = rule(M5, 5, seeds=[3, 1])
    assert picks.tolist() == [3, 1, 0, 4, 2]
    assert ps.tolist() == [0.0, F(.7), F(.3), F(.4), F(.8)]
    picks, ps, rs, nr = rule(M5, 4, seeds=[3, 1])
    assert rs.tolist() == [1.0, 1.0, F(.8), 1.0, 1.0] and nr.tolist() == [2, 1, 3, 0, 3]
    # max_score stops BEFORE a candidate whose maxsim is strictly greater
    assert rule(M5, 5, [3, 1], max_score=0.5)[0].tolist() == [3, 1, 0, 4]
    assert rule(M5, 5, [3, 1], max_score=0.4)[0].tolist() == [3, 1, 0, 4]
    assert rule(M5, 5, [3, 1], max_score=0.35)[0].tolist() == [3, 1, 0]
    assert rule(M5, 5, [3, 1], max_score=0.0)[0].tolist() == [3, 1]
    picks, ps, rs, nr = rule(M5, 2, seeds=[3, 1])  # seeds only
    assert picks.tolist() == [3, 1] and ps.tolist() == [0.0, F(.7)]
    assert rs.tolist() == [F(.3), 1.0, F(.5), 1.0, F(.4)] and nr.tolist() == [0, 1, 0, 0, 1]
    # no seeds: row 0 first
    assert rule(M5, 5)[0].tolist() == [0, 1, 4, 3, 2]


def table4():
    return capi.Table(1024).add_rows(np.arange(4 * 32, dtype=np.uint32).reshape(4, 32))


def test_maxmin_argument_validation_without_a_gpu():
    t = table4()
    bad = [
        dict(npicks=5),                                                  # npicks > N
        dict(npicks=1, seeds=[0, 1]),                                    # nseeds > npicks
        dict(npicks=2, seeds=[4]),                                       # seed outside the table
        dict(npicks=2, seeds=[1, 1]),                                    # repeated seed
        dict(npicks=2, max_score=-0.1), dict(npicks=2, max_score=1.5), dict(npicks=2, max_score=float("nan")),
        dict(npicks=2, metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7),  # asymmetric
        dict(npicks=2, metric=capi.METRIC_TVERSKY, alpha=-0.5, beta=-0.5),
        dict(npicks=2, metric=capi.METRIC_TVERSKY, alpha=float("inf"), beta=float("inf")),
        dict(npicks=2, metric=capi.METRIC_TVERSKY, alpha=float("nan"), beta=float("nan")),
        dict(npicks=2, metric=7),
    ]
    for kw in bad:
        with pytest.raises(capi.GsimError) as e:
            t.maxmin(**kw)
        assert e.value.code == -1, kw
    L = capi.load()
    n = C.c_uint32(0)
    picks = np.zeros(4, np.uint32)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.gsim_db_maxmin(None, 1, None, 0, 0, 1.0, 1.0, 1.0, u32(picks), None, C.byref(n), None, None, None) == -1
    assert L.gsim_db_maxmin(t._h, 1, None, 0, 0, 1.0, 1.0, 1.0, None, None, C.byref(n), None, None, None) == -1
    assert L.gsim_db_maxmin(t._h, 1, None, 0, 0, 1.0, 1.0, 1.0, u32(picks), None, None, None, None, None) == -1
    assert L.gsim_db_maxmin(t._h, 2, None, 1, 0, 1.0, 1.0, 1.0, u32(picks), None, C.byref(n), None, None, None) == -1  # NULL seeds


def test_maxmin_without_a_gpu_is_a_state_error_never_a_host_computation():
    t = table4()
    for kw in (dict(npicks=2), dict(npicks=4, seeds=[2, 0]), dict(npicks=3, metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5),
               dict(npicks=2, assign=True), dict(npicks=4, max_score=0.0)):
        with pytest.raises(capi.GsimError) as e:
            t.maxmin(**kw)
        assert e.value.code == -5, kw
