"""CPU checks of the centroid-clustering calls: the five prototypes and three stats structs against the header; every
GSIM_ERR_INVALID of gsim_db_assign, gsim_db_label_counts and gsim_db_kmeans on tables that are not on a GPU (with a message, the
outputs untouched, an argument error before the state error, a valid call a state error and never a host computation);
gsim_label_centroids against the rule of tests/kmeans_rule.py (sizes 0, 1, 2 -- the tie 2c == n sets the bit -- odd and even sizes,
previous NULL and given, 32 and 4096 bits, a count above its size refused with nothing written); the stand-alone program
tests/cpp/kmeans_host_check.cpp over gsim_label_centroids, built plainly and run.
Not checked here: GSIM_ERR_INVALID for a table of 2^32 rows or more."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kmeans_rule as R
from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
NEW = ["gsim_db_assign", "gsim_db_label_counts", "gsim_label_centroids", "gsim_db_kmeans"]
U32P, F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
FILL = 0xA5A5A5A5


def message():
    return capi.load().gsim_last_error().decode()


def u32(a):
    return a.ctypes.data_as(U32P)


def f32(a):
    return a.ctypes.data_as(F32P)


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


CTYPE = {"gsim_db*": C.c_void_p, "const uint32_t*": U32P, "uint32_t*": U32P, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int,
         "float": C.c_float, "float*": F32P, "gsim_assign_stats*": C.POINTER(capi.GsimAssignStats),
         "gsim_label_stats*": C.POINTER(capi.GsimLabelStats), "gsim_kmeans_stats*": C.POINTER(capi.GsimKmeansStats)}


def test_the_prototypes_and_structs_match_the_header():
    L = capi.load()
    text = header()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert [CTYPE[t] for t in prototype(text, name)] == list(fn.argtypes), name
    assert len(prototype(text, "gsim_db_assign")) == 11 and len(prototype(text, "gsim_db_label_counts")) == 8
    assert len(prototype(text, "gsim_label_centroids")) == 6 and len(prototype(text, "gsim_db_kmeans")) == 12
    scalar = {"uint64_t": C.c_uint64, "double": C.c_double}
    for cname, cls, nfields in (("gsim_assign_stats", capi.GsimAssignStats, 9), ("gsim_label_stats", capi.GsimLabelStats, 8),
                                ("gsim_kmeans_stats", capi.GsimKmeansStats, 7)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for d in body.split(";"):
            if d.strip():
                t, names = d.split(None, 1)
                fields += [(n.strip(), scalar[t]) for n in names.split(",")]
        assert fields == list(cls._fields_), cname
        assert C.sizeof(cls) == 8 * nfields == 8 * len(fields)
    assert re.search(r"#define\s+GSIM_ASSIGN_MAX_CENTRES\s+65536u", text) and capi.ASSIGN_MAX_CENTRES == 65536
    assert re.search(r"#define\s+GSIM_LABEL_NONE\s+0xFFFFFFFFu", text) and capi.LABEL_NONE == capi.LEADER_NONE == 0xFFFFFFFF
    assert capi.Table.assign and capi.Table.label_counts and capi.Table.kmeans and capi.label_centroids
    assert "LOWEST index" in text and "rounded f32 scores" in text


@pytest.fixture(scope="module")
def tables():
    t = capi.Table(1024).add_rows(np.arange(40 * 32, dtype=np.uint32).reshape(40, 32))
    wide = capi.Table(4128).add_rows(np.ones((3, 129), np.uint32))
    empty = capi.Table(1024)
    yield t, wide, empty
    for x in (t, wide, empty):
        x.close()


def test_assign_on_a_table_that_is_not_on_a_gpu(tables):
    L = capi.load()
    t, wide, _ = tables
    cen = np.ones((3, 32), np.uint32)
    label = np.full(40, FILL, np.uint32)
    score = np.full(40, FILL, np.uint32)
    st = capi.GsimAssignStats()
    st.rows = 77
    big = np.zeros((1, 1), np.uint32)  # (never read: m is refused first)
    wcen = np.ones((3, 129), np.uint32)
    nan, inf = float("nan"), float("inf")
    ok = (t._h, u32(cen), 3, 0, 40, 0, 1.0, 1.0, u32(label), f32(score.view(np.float32)), C.byref(st))

    def with_(**kw):
        names = ["db", "centres", "m", "rb", "re", "metric", "alpha", "beta", "label", "score", "stats"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)
    cases = {
        "NULL db": with_(db=None), "m == 0": with_(m=0), "m above the cap": with_(m=65537, centres=u32(big)), "NULL centres": with_(centres=None),
        "NULL label": with_(label=None), "begin past end": with_(rb=5, re=4), "end past the table": with_(re=41),
        "an unknown metric": with_(metric=2), "a negative metric": with_(metric=-1), "Tversky alpha < 0": with_(metric=1, alpha=-0.5),
        "Tversky beta NaN": with_(metric=1, beta=nan), "Tversky alpha infinite": with_(metric=1, alpha=inf),
        "rows wider than 4096 bits": (wide._h, u32(wcen), 3, 0, 3, 0, 1.0, 1.0, u32(label), None, None),
    }
    for what, args in cases.items():
        assert L.gsim_db_assign(*args) == INVALID and len(message()) > 0, what
        assert (label == FILL).all() and (score == FILL).all() and st.rows == 77, what
    assert "4096" in message()
    assert L.gsim_db_assign(*ok) == STATE and "GPU" in message()
    assert L.gsim_db_assign(*with_(rb=3, re=3)) == STATE, "an empty range still needs a table on a GPU"
    assert L.gsim_db_assign(*with_(metric=1, alpha=0.0, beta=0.0)) == STATE, "Tversky (0, 0) is a valid metric"
    assert L.gsim_db_assign(*with_(m=65536, re=41)) == INVALID, "an argument error wins over the state error"
    assert (label == FILL).all() and (score == FILL).all()
    with pytest.raises(capi.GsimError) as e:
        t.assign(cen)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.assign(cen[:0])
    assert e.value.code == INVALID


def test_label_counts_on_a_table_that_is_not_on_a_gpu(tables):
    L = capi.load()
    t, wide, empty = tables
    labels = (np.arange(40) % 5).astype(np.uint32)
    labels[3] = capi.LABEL_NONE
    counts = np.full((5, 1024), FILL, np.uint32)
    sizes = np.full(5, FILL, np.uint32)
    st = capi.GsimLabelStats()
    st.labels = 77
    bad = labels.copy()
    bad[39] = 5
    nearly = labels.copy()
    nearly[0] = 0xFFFFFFFE
    ok = (t._h, u32(labels), 5, 0, 40, u32(counts), u32(sizes), C.byref(st))
    cases = {
        "NULL db": (None,) + ok[1:], "NULL labels": (t._h, None) + ok[2:], "nlabels == 0": ok[:2] + (0,) + ok[3:], "NULL counts": ok[:5] + (None,) + ok[6:],
        "begin past end": ok[:3] + (5, 4) + ok[5:], "end past the table": ok[:3] + (0, 41) + ok[5:], "a label == nlabels": (t._h, u32(bad)) + ok[2:],
        "a label just below NONE": (t._h, u32(nearly)) + ok[2:], "a label above a smaller nlabels": ok[:2] + (4,) + ok[3:],
        "rows wider than 4096 bits": (wide._h, u32(labels), 5, 0, 3, u32(counts), None, None),
    }
    for what, args in cases.items():
        assert L.gsim_db_label_counts(*args) == INVALID and len(message()) > 0, what
        assert (counts == FILL).all() and (sizes == FILL).all() and st.labels == 77, what
    assert L.gsim_db_label_counts(*(ok[:2] + (4,) + ok[3:])) == INVALID and "row 4" in message(), "the first offending row is named"
    assert L.gsim_db_label_counts(*ok) == STATE and "GPU" in message()
    assert L.gsim_db_label_counts(*(ok[:3] + (3, 3) + ok[5:])) == STATE, "an empty range still needs a table on a GPU"
    assert L.gsim_db_label_counts(*((t._h, u32(bad)) + ok[2:])) == INVALID, "an argument error wins over the state error"
    assert (counts == FILL).all() and (sizes == FILL).all()
    with pytest.raises(capi.GsimError) as e:
        t.label_counts(labels, 5)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.label_counts(labels[:39], 5)
    assert e.value.code == INVALID
    # a table without rows has nothing to read: zeros, as gsim_db_bit_counts
    assert L.gsim_db_label_counts(empty._h, None, 5, 0, 0, u32(counts), u32(sizes), None) == OK and not counts.any() and not sizes.any()
    c, z = empty.label_counts([], 3)
    assert c.shape == (3, 1024) and not c.any() and z.tolist() == [0, 0, 0]


def test_kmeans_on_a_table_that_is_not_on_a_gpu(tables):
    L = capi.load()
    t, wide, empty = tables
    init = np.ones((3, 32), np.uint32)
    centres = np.full((3, 32), FILL, np.uint32)
    label = np.full(40, FILL, np.uint32)
    score = np.full(40, FILL, np.uint32)
    sizes = np.full(3, FILL, np.uint32)
    st = capi.GsimKmeansStats()
    st.iterations = 77
    ok = (t._h, u32(init), 3, 10, 0, 1.0, 1.0, u32(centres), u32(label), f32(score.view(np.float32)), u32(sizes), C.byref(st))
    winit = np.ones((3, 129), np.uint32)
    cases = {
        "NULL db": (None,) + ok[1:], "NULL init": (t._h, None) + ok[2:], "m == 0": ok[:2] + (0,) + ok[3:], "m above the cap": ok[:2] + (65537,) + ok[3:],
        "max_iter == 0": ok[:3] + (0,) + ok[4:], "an unknown metric": ok[:4] + (7,) + ok[5:], "Tversky beta < 0": ok[:4] + (1, 1.0, -1.0) + ok[7:],
        "Tversky alpha NaN": ok[:4] + (1, float("nan"), 1.0) + ok[7:], "NULL centres": ok[:7] + (None,) + ok[8:], "NULL label": ok[:8] + (None,) + ok[9:],
        "rows wider than 4096 bits": (wide._h, u32(winit), 3, 10, 0, 1.0, 1.0, u32(winit), u32(label), None, None, None),
    }
    for what, args in cases.items():
        assert L.gsim_db_kmeans(*args) == INVALID and len(message()) > 0, what
        assert (centres == FILL).all() and (label == FILL).all() and (score == FILL).all() and (sizes == FILL).all() and st.iterations == 77, what
    assert L.gsim_db_kmeans(*ok) == STATE and "GPU" in message()
    assert L.gsim_db_kmeans(*(ok[:3] + (0,) + ok[4:])) == INVALID, "an argument error wins over the state error"
    assert L.gsim_db_kmeans(*((empty._h,) + ok[1:])) == STATE
    assert (centres == FILL).all() and (label == FILL).all() and (sizes == FILL).all()
    with pytest.raises(capi.GsimError) as e:
        t.kmeans(init)
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        t.kmeans(init, max_iter=0)
    assert e.value.code == INVALID


@pytest.mark.parametrize("bits", [32, 160, 4096])
def test_label_centroids_follow_the_rule(bits):
    rng = np.random.default_rng(bits)
    sizes = np.array([0, 1, 2, 3, 4, 7, 10, 1001, 2**32 - 1, 0, 2], np.uint32)
    L = len(sizes)
    n = sizes.astype(np.uint64)[:, None]
    pick = rng.integers(0, 5, size=(L, bits))
    counts = np.select([pick == 0, pick == 1, pick == 2, pick == 3],
                       [np.zeros((L, bits), np.uint64), np.broadcast_to(n, (L, bits)), np.broadcast_to(n // 2, (L, bits)),
                        np.broadcast_to(n - n // 2, (L, bits))], (rng.random((L, bits)) * n.astype(np.float64)).astype(np.uint64))
    counts = np.minimum(counts, n).astype(np.uint32)
    prev = rng.integers(0, 2**32, size=(L, bits // 32), dtype=np.uint64).astype(np.uint32)
    for previous in (None, prev):
        want = R.centroids(counts, sizes, previous)
        got = capi.label_centroids(counts, sizes, previous)
        assert got.dtype == np.uint32 and got.shape == (L, bits // 32)
        assert np.array_equal(got, want), (bits, previous is None)
        empty = np.flatnonzero(sizes == 0)
        assert len(empty) == 2 and all(np.array_equal(got[l], prev[l] if previous is not None else np.zeros(bits // 32, np.uint32)) for l in empty)
    # what the rule says at the edges, written out: size 1 copies the row; size 2 is the OR (the tie 2c == n sets the bit); odd sizes
    # need more than half
    c = np.zeros((4, bits), np.uint32)
    c[0, 5], c[1, 5], c[1, 6], c[2, 5], c[2, 6], c[3, 5], c[3, 6] = 1, 1, 2, 1, 2, 3, 4
    got = capi.label_centroids(c, np.array([1, 2, 3, 7], np.uint32))
    assert got[:, 0].tolist() == [1 << 5, (1 << 5) | (1 << 6), 1 << 6, 1 << 6] and not got[:, 1:].any()


def test_label_centroids_refuse_malformed_input():
    L = capi.load()
    counts = np.zeros((2, 64), np.uint32)
    sizes = np.array([3, 0], np.uint32)
    out = np.full((2, 2), FILL, np.uint32)
    counts[0, 9] = 4
    assert L.gsim_label_centroids(u32(counts), u32(sizes), 2, 64, None, u32(out)) == INVALID and "label 0" in message() and (out == FILL).all()
    counts[0, 9] = 3
    counts[1, 63] = 1
    assert L.gsim_label_centroids(u32(counts), u32(sizes), 2, 64, None, u32(out)) == INVALID and "label 1" in message() and (out == FILL).all()
    counts[1, 63] = 0
    for what, args in {"NULL counts": (None, u32(sizes), 2, 64, None, u32(out)), "NULL sizes": (u32(counts), None, 2, 64, None, u32(out)),
                       "NULL centres": (u32(counts), u32(sizes), 2, 64, None, None), "nlabels == 0": (u32(counts), u32(sizes), 0, 64, None, u32(out)),
                       "fp_bits == 0": (u32(counts), u32(sizes), 2, 0, None, u32(out)), "fp_bits no multiple of 32": (u32(counts), u32(sizes), 2, 48, None, u32(out))}.items():
        assert L.gsim_label_centroids(*args) == INVALID and len(message()) > 0, what
        assert (out == FILL).all(), what
    assert L.gsim_label_centroids(u32(counts), u32(sizes), 2, 64, None, u32(out)) == OK and out.tolist() == [[1 << 9, 0], [0, 0]]
    with pytest.raises(capi.GsimError) as e:
        capi.label_centroids(counts, sizes[:1])
    assert e.value.code == INVALID


def test_the_stand_alone_checker_builds_plainly_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "kmeans_host_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "kmeans_host_check")
    libdir = os.path.join(ROOT, "gpusimilarity_amd")
    deps = [src, os.path.join(ROOT, "include", "gpusim_hip.h"), os.path.join(libdir, "libgsim_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + libdir, "-lgsim_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout + r.stderr
