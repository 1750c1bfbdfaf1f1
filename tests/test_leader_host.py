"""CPU checks of gsim_db_leader: the symbol exists, the stats struct and GSIM_LEADER_NONE match the header, the argument errors are
reported before any device state -- on a table that is not on a GPU -- with a message, a valid call on such a table is a state
error (never a host computation), and the numpy restatement of the rule (leader_rule.py, the oracle of tests/test_gpu_leader.py)
on a hand-worked 8-row table.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more -- at the narrowest width such a table is 16 GiB of host rows, more
than a test may build; the check is one comparison in gsim_db_leader, ahead of the state checks like the others."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi
from leader_rule import NONE, leader_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
F = np.float32


def u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbol_exists_and_is_exported():
    L = capi.load()
    assert hasattr(L, "gsim_db_leader")
    assert "gsim_db_leader" in capi.EXPORTS
    assert capi.GsimLeaderStats and capi.Table.leader


def test_stats_struct_and_the_none_value_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_leader_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    names = [n for _, n in fields]
    assert names[:8] == ["leaders", "rounds", "launches", "pairs", "assigned", "kernel_ms", "d2h_ms", "wall_ms"]
    assert names == [n for n, _ in capi.GsimLeaderStats._fields_]
    assert [{"uint64_t": C.c_uint64, "double": C.c_double}[t] for t, _ in fields] == [t for _, t in capi.GsimLeaderStats._fields_]
    assert C.sizeof(capi.GsimLeaderStats) == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_LEADER_NONE\s+0xFFFFFFFFu\b", text)
    assert capi.LEADER_NONE == 0xFFFFFFFF == NONE
    assert re.search(r"int gsim_db_leader\(gsim_db\* db, float cutoff, const uint32_t\* seeds, uint32_t nseeds, uint32_t max_leaders, int metric", text)


class Call:
    """gsim_db_leader on a table that is not on a GPU, one argument changed at a time."""

    def __init__(self, bits=1024, rows=40):
        W = bits // 32
        self.n = rows
        self.t = capi.Table(bits)
        if rows:
            self.t.add_rows(np.arange(rows * W, dtype=np.uint32).reshape(rows, W))
        self.leaders = np.zeros(max(rows, 1), np.uint32)
        self.nleaders = C.c_uint32(77)

    def __call__(self, db=True, cutoff=0.5, seeds=(), null_seeds=False, max_leaders=None, metric=TAN, alpha=1.0, beta=1.0, leaders=True,
                 nleaders=True):
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        return capi.load().gsim_db_leader(
            self.t._h if db else None, cutoff, None if null_seeds or len(sd) == 0 else u32(sd), 3 if null_seeds else len(sd),
            self.n if max_leaders is None else max_leaders, metric, alpha, beta, u32(self.leaders) if leaders else None,
            C.byref(self.nleaders) if nleaders else None, None, None, None)


def test_argument_errors_come_before_any_device_state():
    call = Call()
    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL db": dict(db=False), "NULL leaders": dict(leaders=False), "NULL nleaders": dict(nleaders=False),
        "NULL seeds with nseeds > 0": dict(null_seeds=True),
        "cutoff 0": dict(cutoff=0.0), "cutoff < 0": dict(cutoff=-0.25), "cutoff > 1": dict(cutoff=1.0000001), "cutoff NaN": dict(cutoff=nan),
        "cutoff inf": dict(cutoff=inf),
        "unknown metric": dict(metric=7), "negative metric": dict(metric=-1),
        "asymmetric weights": dict(metric=TV, alpha=0.3, beta=0.7),
        "negative weights": dict(metric=TV, alpha=-0.5, beta=-0.5),
        "infinite weights": dict(metric=TV, alpha=inf, beta=inf), "NaN weights": dict(metric=TV, alpha=nan, beta=nan),
        "a seed past the table": dict(seeds=[3, 40]), "a repeated seed": dict(seeds=[3, 7, 3]),
        "max_leaders 0": dict(max_leaders=0), "max_leaders below the seeds": dict(seeds=[1, 2, 3], max_leaders=2),
        "max_leaders above N": dict(max_leaders=41),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert len(message()) > 0, what
    call.t.set_row_base(100)
    assert call(seeds=[99]) == INVALID and call(seeds=[140]) == INVALID, "seeds carry the row base"
    assert call(seeds=[100, 139]) == STATE
    call.t.close()


def test_rows_wider_than_4096_bits_are_invalid():
    wide = Call(bits=4128, rows=3)
    assert wide() == INVALID and "4096" in message()
    wide.t.close()
    widest = Call(bits=4096, rows=3)
    assert widest() == STATE
    widest.t.close()


def test_an_empty_table_does_nothing():
    empty = Call(rows=0)
    assert empty(max_leaders=0) == OK and empty.nleaders.value == 0
    assert empty(max_leaders=5) == OK and empty.nleaders.value == 0
    assert empty(cutoff=0.0) == INVALID, "an argument error still wins"
    empty.t.close()


def test_a_valid_call_on_a_table_not_on_a_gpu_is_a_state_error():
    call = Call()
    for kw in (dict(), dict(cutoff=1.0), dict(cutoff=1e-6), dict(seeds=[5, 2]), dict(seeds=[39], max_leaders=1), dict(max_leaders=1),
               dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=0.0, beta=0.0), dict(metric=TAN, alpha=-1.0, beta=float("nan"))):
        assert call(**kw) == STATE, kw
        assert "GPU" in message(), kw
        assert call.nleaders.value == 0
    assert call(cutoff=2.0) == INVALID, "an argument error wins over it"
    call.t.close()
    t = capi.Table(1024).add_rows(np.ones((5, 32), np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.leader(0.5)
    assert e.value.code == STATE and len(str(e.value)) > 0
    with pytest.raises(capi.GsimError) as e:
        t.leader(0.5, max_leaders=6)
    assert e.value.code == INVALID
    t.close()


def worked_table():
    """Eight rows, cutoff 0.5.  Rows 5 and 2 (the seeds, in that order) cover each other; row 3 is all-zero (NaN against everything,
    itself included); row 6 is a duplicate of row 0 (the same scores against everything, 1.0 against row 0).  Unlisted pairs: 0.1."""
    nan = float("nan")
    m = np.full((8, 8), 0.1, np.float32)
    np.fill_diagonal(m, 1.0)
    for (i, j), v in {(5, 2): .9, (5, 1): .6, (2, 1): .7, (2, 4): .5, (0, 6): 1.0, (0, 7): .8, (6, 7): .8}.items():
        m[i, j] = m[j, i] = F(v)
    m[3, :] = nan
    m[:, 3] = nan
    return m


def test_the_rule_on_a_hand_worked_table():
    m = worked_table()
    rule = lambda **kw: leader_rule(lambda r: m[r], 8, 0.5, **kw)
    # seeds 5, 2: both leaders although score(5, 2) = .9.  Row 0: .1 against both -> leader 2.  Row 1: covered by both seeds, the
    # earlier one (position 0) keeps it, at .6.  Row 3: NaN -> leader 3, a singleton.  Row 4: exactly .5 against row 2 -> covered,
    # position 1.  Row 6, the duplicate of row 0 -> position 2 at 1.0.  Row 7: .8 against row 0 -> position 2.
    leaders, leader_of, row_score, pairs = rule(seeds=[5, 2])
    assert leaders.tolist() == [5, 2, 0, 3]
    assert leader_of.tolist() == [2, 0, 1, 3, 1, 0, 2, 2]
    assert row_score.tolist() == [1.0, F(.6), 1.0, 1.0, F(.5), 1.0, 1.0, F(.8)]
    # seed 5 meets rows 0 1 3 4 6 7 (6), seed 2 what is left, 0 3 4 6 7 (5), leader 0 meets 3 6 7 (3), leader 3 nobody
    assert pairs == 6 + 5 + 3
    # the cap: leader number 3 is made and covers its rows, then the walk stops -- row 3 stays unassigned
    leaders, leader_of, row_score, pairs = rule(seeds=[5, 2], max_leaders=3)
    assert leaders.tolist() == [5, 2, 0]
    assert leader_of.tolist() == [2, 0, 1, NONE, 1, 0, 2, 2]
    assert row_score.tolist() == [1.0, F(.6), 1.0, 0.0, F(.5), 1.0, 1.0, F(.8)]
    assert pairs == 14
    # a cap equal to the seeds: they cover their rows and that is all
    leaders, leader_of, row_score, pairs = rule(seeds=[5, 2], max_leaders=2)
    assert leaders.tolist() == [5, 2]
    assert leader_of.tolist() == [NONE, 0, 1, NONE, 1, 0, NONE, NONE]
    assert row_score.tolist() == [0.0, F(.6), 1.0, 0.0, F(.5), 1.0, 0.0, 0.0]
    assert pairs == 11
    # no seeds: row 0 leads 6 and 7; row 1 leads 2 (.7) and 5 (.6); row 3; row 4 (.5 against row 2 only, which is no leader)
    leaders, leader_of, row_score, pairs = rule()
    assert leaders.tolist() == [0, 1, 3, 4]
    assert leader_of.tolist() == [0, 1, 1, 2, 3, 1, 0, 0]
    assert row_score.tolist() == [1.0, 1.0, F(.7), 1.0, 1.0, F(.6), 1.0, F(.8)]
    assert pairs == 7 + 4 + 1 + 0
    # just above .5 row 4 no longer joins row 2
    above = float(np.nextafter(F(.5), F(1)))
    leaders, leader_of, _, _ = leader_rule(lambda r: m[r], 8, above, seeds=[5, 2])
    assert leaders.tolist() == [5, 2, 0, 3, 4] and leader_of[4] == 4
