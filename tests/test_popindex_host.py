"""CPU checks of the popcount-index calls: the symbols exist, the stats struct, the flag and the prototypes match the header;
gsim_popcount_bounds equals the numpy restatement of the rule (popindex_rule.py, the oracle of tests/test_gpu_popindex.py) byte for
byte, equals Tanimoto's closed form, and bounds the oracle's score of random fingerprint pairs; every argument error is reported
before any device state -- on a table that is not on a GPU -- as tests/golden/popindex_front_errors.json records it, and a valid
call on such a table is a state error (never a host computation).  tests/cpp/popindex_host_check.cpp, a stand-alone program, runs the
host bound with buffers of exactly the promised size, built plainly and under the address and undefined-behaviour sanitizers.
Not checked: GSIM_ERR_INVALID for a table of 2^32 rows or more (16 GiB of host rows at the narrowest width)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import popindex_front_errors_cases as cases
import popindex_rule as R
from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, TV = capi.METRIC_TANIMOTO, capi.METRIC_TVERSKY
NEW = ["gsim_popindex_create", "gsim_popindex_first", "gsim_popindex_order", "gsim_popindex_destroy", "gsim_popcount_bounds",
       "gsim_db_search_bounded"]
METRICS = [(TAN, 1.0, 1.0), (TV, 1.0, 1.0), (TV, 1.0, 0.0), (TV, 0.5, 0.5), (TV, 0.3, 0.2), (TV, 2.0, 0.5)]
WIDTHS = [64, 160, 1024, 4096]


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.GsimPopindexStats and capi.PopIndex and capi.Table.popindex and capi.Table.search_bounded and capi.popcount_bounds
    assert capi.PopIndex.first and capi.PopIndex.order and capi.PopIndex.__enter__ and capi.PopIndex.__exit__


def test_stats_struct_flag_and_prototypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_popindex_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    assert [n for _, n in fields] == ["rows_scanned", "rows_window", "queries_one_stage", "queries_two_stage", "queries_plain", "launches",
                                      "bounds_ms", "kernel_ms", "wall_ms"]
    base = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, base[t]) for t, n in fields] == list(capi.GsimPopindexStats._fields_)
    assert re.search(r"#define GSIM_POPINDEX_ROWS 1u", text) and capi.POPINDEX_ROWS == 1
    ctype = {"gsim_db*": C.c_void_p, "const gsim_popindex*": C.c_void_p, "gsim_popindex*": C.c_void_p, "gsim_popindex**": C.POINTER(C.c_void_p),
             "uint32_t": C.c_uint32, "int": C.c_int, "float": C.c_float, "const uint32_t*": C.POINTER(C.c_uint32),
             "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64), "float*": C.POINTER(C.c_float), "gsim_hit*": C.c_void_p,
             "gsim_popindex_stats*": C.POINTER(capi.GsimPopindexStats)}
    L = capi.load()
    for name in NEW:
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in proto.split(",")]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and [ctype[t] for t in types] == list(fn.argtypes), name


def test_the_rules_score_is_the_oracles():
    """popindex_rule.score, the vectorised arithmetic the rule's bound is enumerated with, against gso_score_one"""
    rng = np.random.default_rng(0x5C0)
    L = O.lib()
    for metric, alpha, beta in METRICS:
        F = int(rng.choice(WIDTHS))
        a = rng.integers(0, F + 1, 3000)
        b = rng.integers(0, F + 1, 3000)
        c = (rng.random(3000) * (np.minimum(a, b) + 1)).astype(np.int64)
        a[:4], b[:4], c[:4] = [0, 0, F, F], [0, F, 0, F], [0, 0, 0, F]
        got = R.score(metric, alpha, beta, a, b, c)
        want = np.array([L.gso_score_one(metric, alpha, beta, int(x), int(y), int(z)) for x, y, z in zip(a, b, c)], np.float32)
        assert got.tobytes() == want.tobytes(), (metric, alpha, beta)


@pytest.mark.parametrize("bits", WIDTHS)
def test_the_host_bound_is_the_rules_byte_for_byte(bits):
    for metric, alpha, beta in METRICS:
        for a in (0, 1, bits // 2, bits):
            got = capi.popcount_bounds(bits, a, metric, alpha, beta)
            want = R.bounds(bits, a, metric, alpha, beta)
            assert got.dtype == np.float32 and got.shape == (bits + 1,)
            assert got.tobytes() == want.tobytes(), (bits, metric, alpha, beta, a, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5])
            if metric == TAN:
                b = np.arange(bits + 1)
                lo, hi = np.minimum(a, b).astype(np.float32), np.maximum(a, b).astype(np.float32)
                with np.errstate(invalid="ignore"):
                    closed = np.where(hi == 0, np.float32(0), lo / hi).astype(np.float32)
                assert got.tobytes() == closed.tobytes(), (bits, a)


@pytest.mark.parametrize("metric,alpha,beta", METRICS)
def test_no_pair_scores_above_the_bound_of_its_popcounts(metric, alpha, beta):
    """20 000 random (query, row) pairs: the oracle's score is at most ub[popc(row)] of the query's table"""
    rng = np.random.default_rng(0xB0 + int(alpha * 8) + int(beta * 64) + metric)
    W, nq, per = 5, 40, 500  # 160-bit rows; densities from empty to full, so that the overlap's floor a + b - fp_bits matters
    bits = W * 32
    L = O.lib()
    for i in range(nq):
        dq, dr = rng.random(), rng.random(per)
        q = np.packbits(rng.random(bits) < dq, bitorder="little").view(np.uint32)
        rows = np.packbits(rng.random((per, bits)) < dr[:, None], axis=1, bitorder="little").view(np.uint32).reshape(per, W)
        a = int(R.popcounts(q.reshape(1, -1))[0])
        b = R.popcounts(rows)
        c = R.popcounts(rows & q)
        ub = capi.popcount_bounds(bits, a, metric, alpha, beta)
        s = np.array([L.gso_score_one(metric, alpha, beta, a, int(y), int(z)) for y, z in zip(b, c)], np.float32)
        s = np.where(np.isnan(s), np.float32(0), s)
        assert (s <= ub[b]).all(), (i, a)
    assert nq * per == 20000


def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "popindex_front_errors.json")) as f:
        return json.load(f)


def test_every_front_case_answers_as_recorded():
    want = recorded()
    got = json.loads(json.dumps(cases.run_all()))
    assert sorted(got) == sorted(want), "the case list and the recorded file name the same cases"
    assert len(got) >= 40 and {c.split(":")[0] for c in got} == set(cases.ENTRIES)
    wrong = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not wrong, wrong


def test_the_recorded_file_holds_what_it_should():
    """Argument errors are INVALID with a message and come before any device state; a valid call of a device entry point is the state
    error of a table without rows on a GPU; the host function and the destruction of nothing are GSIM_OK."""
    want = recorded()
    for case, r in want.items():
        entry, what = case.split(": ", 1)
        if not what.startswith("valid"):
            assert r["code"] == INVALID and r["message"] and "GPU" not in r["message"], case
        elif entry in ("popcount_bounds", "popindex_destroy"):
            assert r["code"] == OK and r["message"] == "", case
        else:
            assert r["code"] == STATE and r["message"] == "table not finalized (no rows on a GPU)", case
    assert want["popindex_create: NULL db"]["out"]["out"] == "cleared" and want["popindex_create: unknown flags"]["out"]["out"] == "cleared"
    assert want["popindex_create: valid"]["out"]["out"] == "cleared", "*out is cleared on failure"
    assert want["popindex_create: unknown flags"]["message"] == "unknown popcount-index flags"
    assert want["search_bounded: an index made for another handle"]["message"] == "the popcount index was made for another handle"
    for case in ("search_bounded: NULL ix", "search_bounded: unknown metric", "search_bounded: valid"):
        out = want[case]["out"]
        assert out["stats"] == "zero" and out["hits"] == "untouched" and out["counts"] == "untouched" and out["approx"] == "untouched", case
    assert want["search_bounded: valid NULL stats"]["out"]["stats"] is None
    ub = np.array(want["popcount_bounds: valid"]["out"]["ub"], np.uint32).view(np.float32)
    assert ub.tobytes() == R.bounds(32, 3).tobytes()
    assert want["popcount_bounds: fp_bits 33"]["out"]["ub"] == "untouched" and want["popcount_bounds: unknown metric"]["message"] == "unknown metric"
    assert want["popcount_bounds: popcount above fp_bits"]["message"] == "popcount bounds: the query's popcount exceeds fp_bits"


def test_python_wrappers_refuse_a_table_without_a_gpu():
    t = capi.Table(64).add_rows(np.arange(20, dtype=np.uint32).reshape(10, 2))
    with pytest.raises(capi.GsimError) as e:
        t.popindex()
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        capi.popcount_bounds(64, 65)
    assert e.value.code == INVALID
    t.close()


def test_the_stand_alone_checker_builds_plainly_and_under_the_sanitizers_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "popindex_host_check.cpp")
    host = os.path.join(ROOT, "gpusimilarity_amd", "csrc", "capi_popindex_host.cpp")
    deps = [src, host, os.path.join(ROOT, "include", "gpusim_hip.h")]
    common = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    for name, extra in (("popindex_host_check", []),
                        ("popindex_host_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exe = os.path.join(ROOT, "tests", "cpp", name)
        if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
            subprocess.check_call(common + extra + ["-o", exe, src, host])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], (name, r.stdout + r.stderr)
