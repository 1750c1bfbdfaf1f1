"""The fronts of the fifteen single-table calls, and gsim_butina, gsim_components, gsim_mst and gsim_mst_cut, answer every
single-fault input and a handful of valid calls as the commit before their fronts were shared did: the same code, the same
gsim_last_error() bytes, the same outputs cleared, left alone or filled (tests/golden/single_front_errors.json, recorded on that
commit's build by scripts/make_front_errors_golden.py from the case list of single_front_errors_cases.py).  For the valid graphs
the recorded outputs are the result arrays, so the union-find forest and the component numbering are held still too.  No GPU."""
import json
import os

import single_front_errors_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"neighbors", "knn", "maxmin", "leader", "components", "mst", "bit_counts", "overlap_sums", "assign", "label_counts", "kmeans",
           "search_group", "rowset_from_rows", "rowset_from_bitmap", "search_rows"}
QUIRK = ("both infinite", "both -infinite", "both negative")  # gsim_db_neighbors lets these alpha == beta through: kept, DESIGN.md section 25
GRAPHS = {"gsim_butina", "gsim_components", "gsim_mst", "gsim_mst_cut"}


def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "single_front_errors.json")) as f:
        return json.load(f)


def test_every_case_answers_as_recorded():
    want = recorded()
    got = json.loads(json.dumps(cases.run_all()))
    assert sorted(got) == sorted(want), "the case list and the recorded file name the same cases"
    assert len(got) >= 450 and {c.split(":")[0] for c in got} == ENTRIES | GRAPHS
    wrong = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not wrong, wrong


def test_the_recorded_file_holds_what_it_should():
    """Argument errors are INVALID with a message.  A valid call is the state error of a table without rows on a GPU -- or GSIM_OK
    where the call needs no device: on an empty table, and the host functions on a graph, whose outputs are then recorded."""
    want = recorded()
    ok = set()
    for case, r in want.items():
        entry, what = case.split(": ", 1)
        if entry == "neighbors" and what in QUIRK:
            assert r["code"] == -5 and "GPU" in r["message"], case
        elif not what.startswith("valid") and what != "4128-bit rows":
            assert r["code"] == -1 and r["message"] and "GPU" not in r["message"], case
        elif what.startswith("valid Tversky") or what == "4128-bit rows":
            # the metric table of the two-table list is valid here only where the call takes such weights; maxmin, the row sets and
            # the row-set search take rows of any width
            assert r["code"] == (-5 if "GPU" in r["message"] else -1), case
        elif entry in GRAPHS:
            assert r["code"] == 0 and r["message"] == "", case
            ok.add(case)
        elif r["code"] == 0:
            assert "empty table" in what and r["message"] == "", case
            ok.add(case)
        else:
            assert r["code"] == -5 and ("GPU" in r["message"] or what == "valid empty table, a stale row set"), case
    # the empty table answers six calls without a device (k-means and the searches want rows on a GPU first)
    assert {c for c in ok if c.split(":")[0] in ENTRIES} == {e + ": valid empty table" for e in ("leader", "components", "mst", "bit_counts", "overlap_sums",
                                                                                                 "label_counts")}
    # the graph of the case list: the path 0-1-2, the pair 4-5, the lone rows 3 and 6
    comp = want["gsim_components: valid"]["out"]
    assert comp["component_of"] == [0, 0, 0, 1, 2, 2, 3] and comp["first_row"][:4] == [0, 3, 4, 6] and comp["sizes"][:4] == [3, 1, 2, 1]
    assert comp["ncomponents"] == [4, 0]
    cut = want["gsim_mst_cut: valid"]["out"]
    assert cut["component_of"] == [0, 0, 0, 1, 2, 3, 4] and cut["ncomponents"] == [5, 0], "the edge 4-5 scores below the cut"
    assert want["gsim_mst: valid"]["out"]["nedges"] == [3, 0]
    # every message of the shared pieces appears
    texts = {r["message"] for r in want.values()}
    for t in ("NULL seeds", "seed row outside the table", "repeated seed row", "row range: begin past end", "row range outside the table",
              "indptr[0] must be 0", "indptr must not decrease", "NULL indices", "NULL indices or scores", "column index outside the graph",
              "more than 2^32-1 rows", "maxmin: Tversky alpha = beta must be finite and >= 0",
              "neighbour lists need a symmetric metric (Tversky with alpha == beta)"):
        assert t in texts, t
    # the neighbours quirk: alpha == beta is not checked for finiteness there
    for what in QUIRK:
        assert want["neighbors: " + what]["code"] == -5 and want["maxmin: " + what]["code"] == -1, what
