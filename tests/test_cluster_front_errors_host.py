"""The fronts of the ten clustering calls that came after the single-table list (gsim_db_dbscan ... gsim_db_jarvis_patrick), and the
host functions gsim_dbscan, gsim_mreach_mst, gsim_mst_hdbscan, gsim_linkage, gsim_snn and gsim_jarvis_patrick, answer every
single-fault input and a handful of valid calls as the commit before their checks were shared did: the same code, the same
gsim_last_error() bytes, the same outputs cleared, left alone or filled (tests/golden/cluster_front_errors.json, recorded on that
commit's build by scripts/make_front_errors_golden.py from the case list of cluster_front_errors_cases.py).  For the valid host
calls the recorded outputs are the result arrays, so the host rules are held still too.  No GPU."""
import json
import os

import numpy as np

import cluster_front_errors_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"dbscan", "core_scores", "mreach_mst", "hdbscan", "label_sums", "labelset_create", "search_labels", "linkage", "snn", "jarvis_patrick"}
HOST = {"gsim_dbscan", "gsim_mreach_mst", "gsim_mst_hdbscan", "gsim_linkage", "gsim_snn", "gsim_jarvis_patrick"}
FILL, NOISE, MUTUAL = 0xA5A5A5A5, 0xFFFFFFFF, 0x80000000


def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "cluster_front_errors.json")) as f:
        return json.load(f)


def f32(*values):
    return np.array(values, np.float32).view(np.uint32).tolist()


def test_every_case_answers_as_recorded():
    want = recorded()
    got = json.loads(json.dumps(cases.run_all()))
    assert sorted(got) == sorted(want), "the case list and the recorded file name the same cases"
    assert len(got) >= 518 and {c.split(":")[0] for c in got} == ENTRIES | HOST
    wrong = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not wrong, wrong


def test_the_recorded_file_holds_what_it_should():
    """Argument errors are INVALID with a message.  A valid call of a device entry point is the state error of a table without rows
    on a GPU, or GSIM_OK where the call needs no device: on an empty table, and gsim_db_linkage on at most one row.  A valid call of
    a host function is GSIM_OK."""
    want = recorded()
    ok = set()
    for case, r in want.items():
        entry, what = case.split(": ", 1)
        if not what.startswith("valid") and what != "4128-bit rows":
            assert r["code"] == -1 and r["message"] and "GPU" not in r["message"], case
        elif what.startswith("valid Tversky") or what == "4128-bit rows":
            # the metric table of the two-table list is valid here only where the call takes such weights
            assert r["code"] == (-5 if "GPU" in r["message"] else -1), case
        elif entry in HOST:
            assert r["code"] == 0 and r["message"] == "", case
        elif r["code"] == 0:
            assert r["message"] == "", case
            ok.add(case)
        else:
            assert r["code"] == -5 and r["message"] == "table not finalized (no rows on a GPU)", case
    # the device entry points that answer without a device: six on an empty table (label sums, label sets, label searches and
    # gsim_db_snn look at the state first), the dendrogram of at most one row
    empty = ("dbscan", "core_scores", "mreach_mst", "hdbscan", "linkage", "jarvis_patrick")
    assert ok == {e + ": valid empty table" for e in empty} | {
        "core_scores: valid empty table, NULL row outputs", "hdbscan: valid empty table, NULL row outputs",
        "jarvis_patrick: valid empty table, NULL row outputs", "linkage: valid table of one row", "linkage: valid one row, NULL merges",
        "linkage: valid empty range"}
    assert want["jarvis_patrick: valid empty table"]["out"]["nclusters"] == [0, 0, 0] + [FILL] * 5, "the three levels of the call"
    assert want["linkage: valid table of one row"]["out"]["stats"][:2] == [1, 0] and want["linkage: valid empty range"]["out"]["nmerges"] == "zero"

    # the graph of the case list (the path 0-1-2 with scores .5 and .75, the pair 4-5 with .25, the lone rows 3 and 6), min_pts 2
    db = want["gsim_dbscan: valid"]["out"]
    assert db["label_of"] == [0, 0, 0, NOISE, 1, 1, NOISE] and db["anchor"] == [0, 1, 2, NOISE, 4, 5, NOISE]
    assert db["first_row"][:3] == [0, 4, FILL] and db["sizes"][:3] == [3, 2, FILL] and db["nclusters"] == [2, 0]
    mr = want["gsim_mreach_mst: valid"]["out"]
    assert mr["core"] == f32(0.5, 0.75, 0.75, 0, 0.25, 0.25, 0), "the best neighbour's score; 0 for a row without one"
    assert mr["edges"][:9] == [1, 2] + f32(0.75) + [0, 1] + f32(0.5) + [4, 5] + f32(0.25) and mr["edges"][9] == FILL and mr["nedges"] == [3, 0]
    # gsim_mst's forest of that graph, floor .25, clusters of two rows or more: {0, 1, 2} and {4, 5}
    hd = want["gsim_mst_hdbscan: valid"]["out"]
    assert hd["label_of"] == [0, 0, 0, NOISE, 1, 1, NOISE] and hd["nclusters"] == [2, 0]
    assert hd["first_row"][:3] == [0, 4, FILL] and hd["sizes"][:3] == [3, 2, FILL] and hd["birth"][:3] == f32(0.25, 0.25) + [FILL]
    assert hd["leave"] == f32(0.5, 0.75, 0.75, 0, 0.25, 0.25, 0)
    # stability: rows 1 and 2 stay to .75, row 0 to .5, above a birth of .25: 2 x .5 + .25 = 1.25; the pair leaves at its birth
    assert np.array(hd["stability"][:4], np.uint32).view(np.float64).tolist() == [1.25, 0.0]
    # the matrix of the case list: 0-1 at .9, 2-3 at .8; the two pairs meet at the least score between them (complete) or the mean
    for kind, last in (("valid", 0.1), ("valid average", (0.2 + 0.1 + 0.3 + 0.2) / 4)):
        lk = want["gsim_linkage: " + kind]["out"]
        m = np.array(lk["merges"], np.uint32).reshape(3, 8)
        assert m[:, :5].tolist() == [[0, 1, 0, 1, 2], [2, 3, 2, 3, 2], [0, 2, 4, 5, 4]] and lk["nmerges"] == [3, 0], kind
        assert m[:, 5].tolist() == f32(0.9, 0.8, last), kind
    # the lists of the case list: 0, 1, 2 name each other (one shared row a pair, mutual), 3 names 0 (nothing shared, one-sided) and
    # 4, 4 names 3 (mutual, nothing shared)
    assert want["gsim_snn: valid"]["out"]["shared"] == [MUTUAL | 1] * 6 + [0, MUTUAL, MUTUAL]
    assert want["gsim_snn: valid closed"]["out"]["shared"] == [MUTUAL | 3] * 6 + [1, MUTUAL | 2, MUTUAL | 2], "closed: the owners count"
    jp = want["gsim_jarvis_patrick: valid"]["out"]  # kmins 0 and 1: 3-4 link at 0 only
    assert jp["cluster_of"][:14] == [0, 0, 0, 1, 1, 2, 3] + [0, 0, 0, 1, 2, 3, 4] and jp["nclusters"][:3] == [4, 5, FILL]
    assert jp["first_row"][:5] == [0, 3, 5, 6, FILL] and jp["first_row"][7:13] == [0, 3, 4, 5, 6, FILL]
    assert jp["sizes"][:5] == [3, 2, 1, 1, FILL] and jp["sizes"][7:13] == [3, 1, 1, 1, 1, FILL]
    assert want["gsim_jarvis_patrick: valid either"]["out"]["cluster_of"][:7] == [0, 0, 0, 0, 0, 1, 2], "3 names 0: one side suffices"

    # every message of the shared pieces appears, under the name of every call that takes it
    texts = {r["message"] for r in want.values()}
    for name in ("dbscan", "core scores", "mreach mst", "hdbscan", "snn", "jarvis-patrick"):
        assert name + ": the cutoff must be in (0, 1]" in texts and name + ": rows wider than 4096 bits" in texts, name
    for name in ("snn", "jarvis-patrick"):
        assert name + ": k must be in [1, GSIM_KNN_MAX_K = 128]" in texts, name
    for t in ("label sums: rows wider than 4096 bits", "label search: rows wider than 4096 bits", "linkage: rows wider than 4096 bits",
              "core scores needs a symmetric metric (Tversky with alpha == beta)", "hdbscan: Tversky alpha = beta must be finite and >= 0",
              "snn: Tversky alpha and beta must be finite and >= 0", "row range: begin past end", "row range outside the table", "unknown metric",
              "indptr[0] must be 0", "indptr must not decrease", "NULL indices", "NULL indices or scores", "column index outside the graph",
              "more than 2^32-1 rows", "mst: an edge needs a < b < nrows", "mst: an edge with a NaN score",
              "hdbscan: a forest over nrows rows has fewer than nrows edges", "the label set was made for another handle"):
        assert t in texts, t
