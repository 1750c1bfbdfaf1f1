"""The fronts of the two-table calls and gsim_db_knn answer every single-fault input, and a handful of valid calls on tables that are
not on a GPU, as the commit before the fronts were shared did: the same code, the same gsim_last_error() bytes, `*out` cleared in the
same cases (tests/golden/front_errors.json, recorded on that commit's build by scripts/make_front_errors_golden.py from the case
list of front_errors_cases.py).  No GPU."""
import json
import os

import front_errors_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_case_answers_as_recorded():
    with open(os.path.join(ROOT, "tests", "golden", "front_errors.json")) as f:
        want = json.load(f)
    got = cases.run_all()
    assert sorted(got) == sorted(want), "the case list and the recorded file name the same cases"
    assert len(got) >= 300 and {"join", "join_queries", "knn_join", "knn_queries", "knn", "histogram", "histogram_queries", "scores",
                                "scores_device", "scores_queries"} == {c.split(":")[0] for c in got}
    wrong = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not wrong, wrong


def test_the_recorded_file_holds_what_it_should():
    """Argument errors are INVALID with a message, the valid calls are the state error of a table without rows on a GPU, and a graph
    call that was given `out` cleared it -- but for gsim_db_join*'s NULL db, which returns before it looks at `out`."""
    with open(os.path.join(ROOT, "tests", "golden", "front_errors.json")) as f:
        want = json.load(f)
    for case, r in want.items():
        entry, what = case.split(": ", 1)
        assert r["code"] == (-5 if what.startswith("valid") else -1), case
        assert r["message"] and ("GPU" in r["message"]) == what.startswith("valid"), case
        if entry in ("join", "join_queries", "knn_join", "knn_queries", "knn"):
            assert r["out_cleared"] == (None if what == "NULL out" else not (what == "NULL db" and entry.startswith("join"))), case
        else:
            assert r["out_cleared"] is None, case
