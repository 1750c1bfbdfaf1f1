"""CPU checks of the label-grouped search: the four prototypes and the stats struct against the header; every GSIM_ERR_INVALID of
gsim_labelset_create and gsim_db_search_labels that can be reached without a device (with a message, *out cleared, an argument error
before the state error); GSIM_ERR_STATE from both on a table that is not on a GPU, never a host computation; and the rule itself
(tests/search_labels_rule.py) against its own three identities on a 300-row table, through oracle_lib alone.
Not checked here: GSIM_ERR_INVALID for a table of 2^32 rows or more.  A label set exists only for a table on a GPU, so what
gsim_db_search_labels checks behind its NULL checks -- another handle's label set, the metric, alpha / beta, the row width, and its own
GSIM_ERR_STATE -- cannot be reached without a device: tests/test_gpu_search_labels.py has those."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import search_labels_rule as R
from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
NEW = ["gsim_labelset_create", "gsim_labelset_sizes", "gsim_labelset_destroy", "gsim_db_search_labels"]
U32P, U64P, VP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p
NONE = 0xFFFFFFFF


def message():
    return capi.load().gsim_last_error().decode()


def u32(a):
    return a.ctypes.data_as(U32P)


def header():
    return open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()


def prototype(text, name):
    """the parameter types of `name` in the header, comments and parameter names removed"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1)
    out = []
    for a in args.split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\b[a-z_0-9]+$", "", a).replace(" *", "*"))
    return out


CTYPE = {"gsim_db*": VP, "const gsim_labelset*": VP, "gsim_labelset*": VP, "gsim_labelset**": C.POINTER(VP), "gsim_hit*": VP, "const uint32_t*": U32P,
         "uint32_t*": U32P, "uint64_t*": U64P, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int, "float": C.c_float,
         "gsim_label_search_stats*": C.POINTER(capi.GsimLabelSearchStats)}


def test_the_names_are_exported_and_documented():
    L = capi.load()
    text = header()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert [CTYPE[t] for t in prototype(text, name)] == list(fn.argtypes), name
    assert len(prototype(text, "gsim_db_search_labels")) == 18 and len(prototype(text, "gsim_labelset_create")) == 4
    assert len(prototype(text, "gsim_labelset_sizes")) == 4 and len(prototype(text, "gsim_labelset_destroy")) == 1
    body = re.search(r"typedef struct \{([^}]*)\} gsim_label_search_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    scalar = {"uint64_t": C.c_uint64, "double": C.c_double}
    fields = []
    for d in body.split(";"):
        if d.strip():
            t, names = d.split(None, 1)
            fields += [(n.strip(), scalar[t]) for n in names.split(",")]
    assert fields == list(capi.GsimLabelSearchStats._fields_)
    assert [f for f, _ in fields] == ["queries", "labels", "passes", "passes_lds", "passes_global", "launches", "scan_ms", "finish_ms", "d2h_ms", "wall_ms"]
    assert C.sizeof(capi.GsimLabelSearchStats) == 8 * 10
    assert "typedef struct gsim_labelset gsim_labelset;" in text
    assert capi.Table.labelset and capi.Table.search_labels and capi.LabelSet.sizes and capi.LabelSet.close and capi.LabelSet.__enter__
    for phrase in ("gsim_db_search_labels, THE RESULT RULE", "row = 0xFFFFFFFF", "with labels[r] = r", "with one label", "gsim_db_search_rows at k = 1",
                   "no environment knob", "tile x nlabels x 24 bytes", "byte-identical from run to run"):
        assert phrase in text, phrase


@pytest.fixture(scope="module")
def tables():
    t = capi.Table(1024).add_rows(np.arange(40 * 32, dtype=np.uint32).reshape(40, 32))
    wide = capi.Table(4128).add_rows(np.ones((3, 129), np.uint32))
    yield t, wide
    for x in (t, wide):
        x.close()


def test_labelset_create_on_a_table_that_is_not_on_a_gpu(tables):
    L = capi.load()
    t, _ = tables
    labels = (np.arange(40) % 5).astype(np.uint32)
    labels[3] = NONE
    bad = labels.copy()
    bad[39] = 5
    nearly = labels.copy()
    nearly[0] = 0xFFFFFFFE
    marker = 0x1234
    cases = {"NULL db": (None, u32(labels), 5), "nlabels == 0": (t._h, u32(labels), 0), "NULL labels": (t._h, None, 5),
             "a label == nlabels": (t._h, u32(bad), 5), "a label just below NONE": (t._h, u32(nearly), 5), "a label above a smaller nlabels": (t._h, u32(labels), 4)}
    for what, args in cases.items():
        out = VP(marker)
        assert L.gsim_labelset_create(*args, C.byref(out)) == INVALID and len(message()) > 0, what
        assert not out.value, (what, "*out is cleared on failure")
    assert L.gsim_labelset_create(t._h, u32(labels), 4, C.byref(VP())) == INVALID and "row 4" in message(), "the first offending row is named"
    assert L.gsim_labelset_create(t._h, u32(labels), 5, None) == INVALID, "NULL out"
    out = VP(marker)
    assert L.gsim_labelset_create(t._h, u32(labels), 5, C.byref(out)) == STATE and "GPU" in message() and not out.value
    assert L.gsim_labelset_create(t._h, u32(bad), 5, C.byref(out)) == INVALID, "an argument error wins over the state error"
    with pytest.raises(capi.GsimError) as e:
        t.labelset(labels, 5)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.labelset(labels[:39], 5)
    assert e.value.code == INVALID
    sizes = np.zeros(5, np.uint32)
    assert L.gsim_labelset_sizes(None, u32(sizes), None, None) == INVALID
    assert L.gsim_labelset_destroy(None) == OK, "destroying nothing is legal, as gsim_rowset_destroy"


def test_search_labels_on_a_table_that_is_not_on_a_gpu(tables):
    """No label set can exist for a table that is not on a GPU, so the label set is a stand-in that only a call which passes the NULL
    checks would look at: every case below has to fail on an argument that is checked before it."""
    L = capi.load()
    t, wide = tables
    q = np.zeros((2, 32), np.uint32)
    hits = np.zeros((2, 4), capi.HIT_DTYPE)
    hit_labels = np.full((2, 4), 77, np.uint32)
    counts = np.full(2, 77, np.uint32)
    st = capi.GsimLabelSearchStats()
    st.queries = 77
    names = ["db", "ls", "queries", "nq", "k", "cutoff", "metric", "alpha", "beta", "launch_rows", "hits", "hit_labels", "counts", "approx", "rows_kept",
             "label_best", "label_kept", "stats"]
    ok = [t._h, None, u32(q), 2, 4, 0.0, 0, 1.0, 1.0, 0, hits.ctypes.data_as(VP), u32(hit_labels), u32(counts), None, None, None, None, C.byref(st)]

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)
    for what, args in {"NULL ls": with_(), "NULL db": with_(db=None), "NULL ls on a wide table": with_(db=wide._h)}.items():
        assert L.gsim_db_search_labels(*args) == INVALID and len(message()) > 0, what
        assert (counts == 77).all() and (hit_labels == 77).all() and st.queries == 77, what
    with pytest.raises(capi.GsimError) as e:
        t.search_labels(capi.LabelSet(t, None, 5), q, 4)
    assert e.value.code == INVALID, "a closed label set is a NULL label set"


def test_the_rule_satisfies_its_three_identities():
    """300 Morgan-shaped rows with an all-zero row, an all-ones row and three identical rows; Tanimoto and Tversky 0.3 / 0.7; cutoffs
    0, negative, dense, selective and 1.0 -- against the oracle's own search on the whole table and on each label's rows."""
    n, W = 300, 32
    db = O.synth_rows(41, O.KIND_MORGAN, 0, n, W)
    db[0] = 0
    db[1] = 0xFFFFFFFF
    db[[2, 3, 4]] = db[10]
    queries = np.stack([db[10], db[77], np.zeros(W, np.uint32)])
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 9, n).astype(np.uint32)
    labels[rng.choice(n, 30, replace=False)] = NONE
    labels[[2, 3, 4]] = (5, 5, 5)
    live = np.flatnonzero(labels != NONE)
    for kw in ({}, dict(metric=O.METRIC_TVERSKY, alpha=0.3, beta=0.7)):
        H = R.pair_hits(db, queries, kw)
        okw = (kw.get("metric", O.METRIC_TANIMOTO), kw.get("alpha", 1.0), kw.get("beta", 1.0))
        sel = float(np.median(H["score"][1][H["score"][1] > 0]))
        for cutoff in (0.0, -1.0, 2.0 ** -20, sel, 1.0):
            for q in range(len(queries)):
                # labels[r] = r: gsim_db_search itself
                for k in (0, 1, 25, 400):
                    w = R.one_query(H[q], np.arange(n, dtype=np.uint32), n, k, cutoff, row_base=1000)
                    hits, approx = O.search(queries[q], db, k, cutoff, *okw, row_base=1000)
                    hits = hits[:min(k, approx)]
                    assert w["count"] == len(hits) and w["approx"] == approx == w["rows_kept"]
                    assert w["hits"].tobytes() == hits.tobytes() and np.array_equal(w["hit_labels"], hits["row"] - 1000)
                # one label: gsim_db_search at k = 1
                w = R.one_query(H[q], np.zeros(n, np.uint32), 1, 5, cutoff)
                hits, approx = O.search(queries[q], db, 1, cutoff, *okw)
                hits = hits[:min(1, approx)]
                assert w["count"] == len(hits) == w["approx"] and w["rows_kept"] == approx and w["hits"].tobytes() == hits.tobytes()
                assert w["label_kept"].tolist() == [approx]
                # every label: the oracle's search on that label's rows alone, k = 1
                w = R.one_query(H[q], labels, 9, 9, cutoff)
                for l in range(9):
                    rows = np.flatnonzero(labels == l)
                    hits, approx = O.search(queries[q], db[rows], 1, cutoff, *okw)
                    assert w["label_kept"][l] == approx
                    if approx:
                        hits["row"] = rows[hits["row"]]
                        assert w["label_best"][l].tobytes() == hits[0].tobytes()
                    else:
                        assert w["label_best"][l] == R.NO_HIT
                assert w["rows_kept"] == w["label_kept"].sum() and w["approx"] == (w["label_kept"] > 0).sum()
                if cutoff <= 0:
                    assert w["rows_kept"] == len(live) and np.array_equal(w["label_kept"], np.bincount(labels[live], minlength=9))
                # the ranking: the bests in canonical order, their labels beside them
                key = [(-float(h["score"]), int(h["row"])) for h in w["hits"]]
                assert key == sorted(key) and len(set(w["hit_labels"].tolist())) == w["count"] == min(9, w["approx"])
                assert all(w["label_best"][l] == h for l, h in zip(w["hit_labels"], w["hits"]))
        # the tie inside a label: rows 2, 3, 4 and 10 are identical, label 5 keeps the lowest of its three
        w = R.one_query(H[0], labels, 9, 9, 1.0)
        assert w["label_best"][5]["row"] == 2 and w["label_best"][5]["score"] == 1.0 and w["label_kept"][5] >= 3
