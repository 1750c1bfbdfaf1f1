"""CPU checks of the label sums: the three prototypes, the flag and the stats struct against the header; every GSIM_ERR_INVALID of
gsim_db_label_sums on a table that is not on a GPU (with a message, the outputs untouched, an argument error before the state error, a
valid call a state error and never a host computation); gsim_label_silhouette and gsim_label_medoids against tests/label_sums_rule.py
bit for bit on hand-made inputs (singletons, an empty label, GSIM_LABEL_NONE rows, one label only, a == b, a == b == 1.0 where d is 0,
medoid ties, sums above 2^53) and on random ones; the rule itself against a plain float64 silhouette of the unquantised scores on a
600-row table with three planted clusters; the stand-alone program tests/cpp/label_sums_host_check.cpp, built with the two host
functions' own file under -fsanitize=address,undefined (static runtimes: nothing is preloaded, nothing goes into python) and run.
Not checked here: GSIM_ERR_INVALID for a table of 2^32 rows or more."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import label_sums_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
NEW = ["gsim_db_label_sums", "gsim_label_silhouette", "gsim_label_medoids"]
U32P, U64P, F64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
NONE = 0xFFFFFFFF
FILL = 0xA5A5A5A5
ONE = 1 << 31


def message():
    return capi.load().gsim_last_error().decode()


def u32(a):
    return a.ctypes.data_as(U32P)


def u64(a):
    return a.ctypes.data_as(U64P)


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


CTYPE = {"gsim_db*": C.c_void_p, "const uint32_t*": U32P, "uint32_t*": U32P, "const uint64_t*": U64P, "uint64_t*": U64P, "uint32_t": C.c_uint32,
         "uint64_t": C.c_uint64, "int": C.c_int, "float": C.c_float, "double*": F64P, "gsim_label_sums_stats*": C.POINTER(capi.GsimLabelSumsStats)}


def test_the_names_are_exported_and_documented():
    L = capi.load()
    text = header()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert [CTYPE[t] for t in prototype(text, name)] == list(fn.argtypes), name
    assert len(prototype(text, "gsim_db_label_sums")) == 15 and len(prototype(text, "gsim_label_silhouette")) == 10
    assert len(prototype(text, "gsim_label_medoids")) == 5
    body = re.search(r"typedef struct \{([^}]*)\} gsim_label_sums_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    scalar = {"uint64_t": C.c_uint64, "double": C.c_double}
    fields = []
    for d in body.split(";"):
        if d.strip():
            t, names = d.split(None, 1)
            fields += [(n.strip(), scalar[t]) for n in names.split(",")]
    assert fields == list(capi.GsimLabelSumsStats._fields_)
    assert [f for f, _ in fields] == ["rows", "rows_labelled", "labels_nonempty", "pairs", "launches", "sort_ms", "gather_ms", "kernel_ms", "d2h_ms",
                                      "wall_ms", "clock_mhz"]
    assert C.sizeof(capi.GsimLabelSumsStats) == 8 * 11
    assert re.search(r"#define\s+GSIM_LABEL_SUMS_OWN_ONLY\s+1u", text) and capi.LABEL_SUMS_OWN_ONLY == 1
    assert capi.Table.label_sums and capi.label_silhouette and capi.label_medoids
    assert "gsim_db_label_sums, THE RESULT RULE" in text and "floor(s * 2^31)" in text and "LOWEST label" in text
    assert "0x1p-31" in text and "LOWEST row" in text and "32 bytes a row of carried state" in text


@pytest.fixture(scope="module")
def tables():
    t = capi.Table(1024).add_rows(np.arange(40 * 32, dtype=np.uint32).reshape(40, 32))
    wide = capi.Table(4128).add_rows(np.ones((3, 129), np.uint32))
    yield t, wide
    for x in (t, wide):
        x.close()


def test_label_sums_on_a_table_that_is_not_on_a_gpu(tables):
    L = capi.load()
    t, wide = tables
    labels = (np.arange(40) % 5).astype(np.uint32)
    labels[3] = NONE
    own = np.full(40, FILL, np.uint64)
    other = np.full(40, FILL, np.uint32)
    other_q = np.full(40, FILL, np.uint64)
    sizes = np.full(5, FILL, np.uint32)
    st = capi.GsimLabelSumsStats()
    st.rows = 77
    bad = labels.copy()
    bad[39] = 5
    nearly = labels.copy()
    nearly[0] = 0xFFFFFFFE
    names = ["db", "labels", "nlabels", "rb", "re", "metric", "alpha", "beta", "flags", "launch_pairs", "own", "other", "other_q", "sizes", "stats"]
    ok = (t._h, u32(labels), 5, 0, 40, 0, 1.0, 1.0, 0, 0, u64(own), u32(other), u64(other_q), u32(sizes), C.byref(st))

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)
    nan, inf = float("nan"), float("inf")
    cases = {
        "NULL db": with_(db=None), "NULL own_q": with_(own=None), "NULL other_label": with_(other=None), "NULL other_q": with_(other_q=None),
        "NULL other_label, an unknown flag beside own-only": with_(other=None, flags=3), "nlabels == 0": with_(nlabels=0), "NULL labels": with_(labels=None),
        "a label == nlabels": with_(labels=u32(bad)), "a label just below NONE": with_(labels=u32(nearly)), "a label above a smaller nlabels": with_(nlabels=4),
        "an unknown flag bit": with_(flags=2), "a high flag bit": with_(flags=0x80000000), "begin past end": with_(rb=5, re=4),
        "end past the table": with_(re=41), "an unknown metric": with_(metric=2), "a negative metric": with_(metric=-1),
        "Tversky alpha < 0": with_(metric=1, alpha=-0.5), "Tversky beta NaN": with_(metric=1, beta=nan), "Tversky alpha infinite": with_(metric=1, alpha=inf),
        "rows wider than 4096 bits": (wide._h, u32(labels), 5, 0, 3, 0, 1.0, 1.0, 0, 0, u64(own), u32(other), u64(other_q), None, None),
    }
    for what, args in cases.items():
        assert L.gsim_db_label_sums(*args) == INVALID and len(message()) > 0, what
        assert (own == FILL).all() and (other == FILL).all() and (other_q == FILL).all() and (sizes == FILL).all() and st.rows == 77, what
    assert "4096" in message()
    assert L.gsim_db_label_sums(*with_(nlabels=4)) == INVALID and "row 4" in message(), "the first offending row is named"
    assert L.gsim_db_label_sums(*ok) == STATE and "GPU" in message()
    assert L.gsim_db_label_sums(*with_(flags=1, other=None, other_q=None)) == STATE, "own-only needs neither other_label nor other_q"
    assert L.gsim_db_label_sums(*with_(metric=1, alpha=0.0, beta=0.0)) == STATE, "Tversky (0, 0) is a valid metric"
    assert L.gsim_db_label_sums(*with_(rb=3, re=3)) == STATE, "an empty range still needs a table on a GPU"
    assert L.gsim_db_label_sums(*with_(labels=u32(bad))) == INVALID, "an argument error wins over the state error"
    assert (own == FILL).all() and (other == FILL).all() and (other_q == FILL).all() and (sizes == FILL).all()
    with pytest.raises(capi.GsimError) as e:
        t.label_sums(labels, 5)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.label_sums(labels, 5, own_only=True, launch_pairs=1 << 14)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.label_sums(labels[:39], 5)
    assert e.value.code == INVALID


def same_bits(got, want):
    return np.array_equal(np.asarray(got, np.float64).view(np.uint64), np.asarray(want, np.float64).view(np.uint64))


def check_host_functions(labels, own, other, other_q, sizes):
    labels, own, other, other_q, sizes = (np.asarray(labels, np.uint32), np.asarray(own, np.uint64), np.asarray(other, np.uint32),
                                          np.asarray(other_q, np.uint64), np.asarray(sizes, np.uint32))
    sil, lmean, mean = capi.label_silhouette(labels, own, other, other_q, sizes)
    wsil, wlmean, wmean = R.silhouette(labels, own, other, other_q, sizes)
    assert same_bits(sil, wsil), (sil, wsil)
    assert same_bits(lmean, wlmean) and same_bits([mean], [wmean])
    med = capi.label_medoids(labels, own, len(sizes))
    assert np.array_equal(med, R.medoids(labels, own, len(sizes)))
    return sil, lmean, mean, med


def test_silhouettes_and_medoids_follow_the_rule_on_hand_made_inputs():
    # label 0: rows 0, 2, 5; label 1: row 1 (a singleton); label 2: empty; label 3: rows 3, 6; row 4: NONE
    labels = [0, 1, 0, 3, NONE, 0, 3]
    sizes = [3, 1, 0, 2]
    own = [ONE, 0, (1 << 62) + 12345, ONE, 0, 2 * ONE, ONE]
    other = [3, 0, 1, 0, NONE, 3, NONE]
    other_q = [ONE, 7, 3, 3 * ONE, 0, ONE // 2, 0]
    sil, lmean, mean, med = check_host_functions(labels, own, other, other_q, sizes)
    assert sil[0] == 0.0, "a == b == 0.5"
    assert sil[1] == 0.0, "a singleton"
    assert sil[2] > 2.0 ** 29, "a sum above 2^53 (no table gives it)"
    assert sil[3] == 0.0, "a == b == 1.0: d is 0"
    assert sil[4] == 0.0, "a GSIM_LABEL_NONE row"
    assert sil[5] == 1.0, "a = 1.0, b = 0.25"
    assert sil[6] == 0.0, "a row without another cluster"
    assert lmean[1] == 0.0 and lmean[2] == 0.0 and lmean[3] == 0.0 and mean == (sil[0] + sil[2] + sil[5]) / 6.0
    assert med.tolist() == [2, 1, NONE, 3], "label 3: rows 3 and 6 tie, the lower row wins"
    # sums above 2^53 whose conversion to double rounds: odd multiples of half an ulp go to even
    big = [(1 << 53) + 1, (1 << 53) + 3, (1 << 60) + 128, (1 << 60) + 384]
    check_host_functions([0, 0, 1, 1], big, [1, 1, 0, 0], big[::-1], [2, 2])
    assert float(np.float64(np.uint64(big[0]))) == 2.0 ** 53 and float(np.float64(np.uint64(big[1]))) == 2.0 ** 53 + 4
    # one label only; every row NONE; no rows
    check_host_functions([0] * 5, [0] * 5, [NONE] * 5, [0] * 5, [5])
    sil, lmean, mean, med = check_host_functions([NONE] * 4, [0] * 4, [NONE] * 4, [0] * 4, [0, 0])
    assert not sil.any() and not lmean.any() and mean == 0.0 and med.tolist() == [NONE, NONE]
    sil, lmean, mean, med = check_host_functions([], [], [], [], [0, 0, 0])
    assert len(sil) == 0 and mean == 0.0 and med.tolist() == [NONE] * 3
    # medoid ties in every label: the lowest row
    med = capi.label_medoids([2, 2, 0, 0, 2, 0], [9, 9, 4, 4, 9, 4], 3)
    assert med.tolist() == [2, NONE, 0]


def test_silhouettes_and_medoids_follow_the_rule_on_random_inputs():
    rng = np.random.default_rng(29)
    for n, nlabels in ((1, 1), (50, 3), (400, 40), (400, 600)):
        labels = rng.integers(0, nlabels, n).astype(np.uint32)
        labels[rng.random(n) < 0.1] = NONE
        sizes = np.bincount(labels[labels != NONE], minlength=nlabels).astype(np.uint32)
        present = np.flatnonzero(sizes)
        own = (rng.integers(0, ONE, n, dtype=np.uint64) * np.maximum(sizes[np.minimum(labels, nlabels - 1)], 1).astype(np.uint64))
        own[rng.random(n) < 0.2] //= np.uint64(7)  # (ties among the sums are rare: make the values coarse for some)
        other = np.full(n, NONE, np.uint32)
        other_q = np.zeros(n, np.uint64)
        for i in range(n):
            cand = present[present != labels[i]]
            if labels[i] != NONE and len(cand):
                other[i] = rng.choice(cand)
                other_q[i] = int(rng.integers(0, ONE)) * int(sizes[other[i]])
        check_host_functions(labels, own, other, other_q, sizes)


def test_the_host_functions_refuse_malformed_input():
    L = capi.load()
    labels = np.array([0, 1, 0, 3, NONE, 0, 3], np.uint32)
    sizes = np.array([3, 1, 0, 2], np.uint32)
    own = np.arange(7, dtype=np.uint64)
    other = np.array([3, 0, 1, 0, NONE, 3, NONE], np.uint32)
    other_q = np.arange(7, dtype=np.uint64)
    sil = np.full(7, 77.0)
    lmean = np.full(4, 77.0)
    mean = C.c_double(77.0)
    names = ["labels", "own", "other", "other_q", "sizes", "n", "nlabels", "sil", "lmean", "mean"]
    ok = (u32(labels), u64(own), u32(other), u64(other_q), u32(sizes), 7, 4, sil.ctypes.data_as(F64P), lmean.ctypes.data_as(F64P), C.byref(mean))

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    cases = {
        "NULL labels": with_(labels=None), "NULL own_q": with_(own=None), "NULL other_label": with_(other=None), "NULL other_q": with_(other_q=None),
        "NULL sizes": with_(sizes=None), "NULL sil": with_(sil=None), "nlabels == 0": with_(nlabels=0),
        "a label == nlabels": with_(labels=u32(changed(labels, 6, 4))), "an other_label equal to the own": with_(other=u32(changed(other, 0, 0))),
        "an other_label == nlabels": with_(other=u32(changed(other, 0, 4))), "an other_label without rows": with_(other=u32(changed(other, 0, 2))),
        "an other_label on a NONE row": with_(other=u32(changed(other, 4, 0))), "sizes that disagree": with_(sizes=u32(changed(sizes, 3, 3))),
        "sizes that disagree on an empty label": with_(sizes=u32(changed(sizes, 2, 1))),
    }
    for what, args in cases.items():
        assert L.gsim_label_silhouette(*args) == INVALID and len(message()) > 0, what
        assert (sil == 77.0).all() and (lmean == 77.0).all() and mean.value == 77.0, what
    assert L.gsim_label_silhouette(*ok) == OK and mean.value != 77.0
    assert L.gsim_label_silhouette(*with_(lmean=None, mean=None)) == OK
    med = np.full(4, FILL, np.uint32)
    for what, args in {"NULL labels": (None, u64(own), 7, 4, u32(med)), "NULL own_q": (u32(labels), None, 7, 4, u32(med)),
                       "NULL medoid": (u32(labels), u64(own), 7, 4, None), "nlabels == 0": (u32(labels), u64(own), 7, 0, u32(med)),
                       "a label == nlabels": (u32(changed(labels, 6, 4)), u64(own), 7, 4, u32(med)),
                       "2^32 rows": (u32(labels), u64(own), 1 << 32, 4, u32(med))}.items():
        assert L.gsim_label_medoids(*args) == INVALID and len(message()) > 0, what
        assert (med == FILL).all(), what
    assert L.gsim_label_medoids(u32(labels), u64(own), 7, 4, u32(med)) == OK and med.tolist() == [5, 1, NONE, 6]
    with pytest.raises(capi.GsimError):
        capi.label_silhouette(labels, own[:6], other, other_q, sizes)
    with pytest.raises(capi.GsimError):
        capi.label_medoids(labels, own[:6], 4)


def test_the_rule_agrees_with_a_float64_silhouette_on_planted_clusters():
    """600 rows in three planted clusters (a centre each, every row its centre with a twentieth of the bits redrawn).  The rule's
    silhouette differs from the plain float64 one of the unquantised scores by the quantisation alone: below 2^-31 in either mean, so
    with d = 1 - min(a, b) >= 0.1 (asserted on the float64 values) below about 2 * 2^-31 / 0.1 + 2^-31 / 0.1^2 = 6e-8 < 1e-6."""
    rng = np.random.default_rng(600)
    n, W = 600, 32
    centres = O.synth_rows(29, O.KIND_MORGAN, 0, 3, W)
    truth = (np.arange(n) % 3).astype(np.uint32)
    noise = O.synth_rows(30, O.KIND_MORGAN, 10, n, W)
    redraw = np.zeros((n, W), np.uint32)
    for b in range(32):
        redraw |= (rng.random((n, W)) < 0.05).astype(np.uint32) << np.uint32(b)
    db = (centres[truth] & ~redraw) | (noise & redraw)
    S = R.score_matrix(db)
    own, other, other_q, sizes, _ = R.sums(S, truth, 3)
    assert sizes.tolist() == [200, 200, 200] and (other != NONE).all()
    sil, lmean, mean = R.silhouette(truth, own, other, other_q, sizes)
    D = S.astype(np.float64)
    np.fill_diagonal(D, 0.0)
    means = np.stack([D[:, truth == l].sum(axis=1) for l in range(3)], axis=1)
    means /= np.where(np.arange(3)[None, :] == truth[:, None], 199.0, 200.0)
    a = means[np.arange(n), truth]
    rest = means.copy()
    rest[np.arange(n), truth] = -1.0
    b = rest.max(axis=1)
    d = 1.0 - np.minimum(a, b)
    assert (d >= 0.1).all(), float(d.min())
    plain = (a - b) / d
    assert float(np.abs(sil - plain).max()) <= 1e-6, float(np.abs(sil - plain).max())
    assert (np.argmax(rest, axis=1) == other).all()
    assert mean > 0.2 and (lmean > 0.2).all(), "the planted clusters are clusters"
    csil, clmean, cmean = capi.label_silhouette(truth, own, other, other_q, sizes)
    assert same_bits(csil, sil) and same_bits(clmean, lmean) and same_bits([cmean], [mean])
    med = capi.label_medoids(truth, own, 3)
    assert np.array_equal(med, R.medoids(truth, own, 3)) and (truth[med] == np.arange(3)).all()


def test_the_stand_alone_checker_builds_under_the_sanitizers_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "label_sums_host_check.cpp")
    host = os.path.join(ROOT, "gpusimilarity_amd", "csrc", "capi_label_sums_host.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "label_sums_host_check")
    deps = [src, host, os.path.join(ROOT, "include", "gpusim_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src, host])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout + r.stderr
