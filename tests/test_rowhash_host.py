"""CPU checks of the row-hash calls: the symbols exist, the stats struct, the constants and the prototypes match the header;
gsim_row_hash equals the numpy restatement of the header's hash (rowhash_rule.py, the oracle of tests/test_gpu_rowhash.py) byte for
byte and depends on a word's position; gsim_duplicates equals the rule; every argument error is reported before any device state --
on a table that is not on a GPU -- as tests/golden/rowhash_front_errors.json records it, and a valid device call on such a table is
a state error (never a host computation).  tests/cpp/rowhash_host_check.cpp, a stand-alone program, runs the host functions with
buffers of exactly the promised sizes, built plainly and under the address and undefined-behaviour sanitizers.
Not checked: GSIM_ERR_INVALID for a table of 2^32 - 1 rows or more (16 GiB of host rows at the narrowest width)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rowhash_front_errors_cases as cases
import rowhash_rule as R
from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
NEW = ["gsim_rowhash_create", "gsim_rowhash_get_stats", "gsim_rowhash_groups", "gsim_rowhash_rowset", "gsim_rowhash_find",
       "gsim_rowhash_find_db", "gsim_rowhash_destroy", "gsim_row_hash", "gsim_duplicates"]
WIDTHS = [32, 96, 160, 1024, 1152, 32768]


def test_the_symbols_exist_and_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.GsimRowhashStats and capi.RowHash and capi.Table.rowhash and capi.row_hash and capi.duplicates
    for method in ("groups", "stats", "rowset", "find", "find_db", "__enter__", "__exit__"):
        assert getattr(capi.RowHash, method)


def test_stats_struct_constants_and_prototypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_rowhash_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert len(fields) == len(re.findall(r";", body)), "uint64_t and double fields only, as the other stats structs"
    assert [n for _, n in fields] == ["rows", "groups", "repeated_groups", "largest_group", "slots", "launches", "kernel_ms", "wall_ms"]
    base = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, base[t]) for t, n in fields] == list(capi.GsimRowhashStats._fields_)
    assert re.search(r"#define GSIM_ROW_NONE 0xFFFFFFFFu", text) and capi.ROW_NONE == R.ROW_NONE == 0xFFFFFFFF
    assert re.search(r"#define GSIM_ROWHASH_REPEATS 1u", text) and capi.ROWHASH_REPEATS == 1
    ctype = {"gsim_db*": C.c_void_p, "const gsim_rowhash*": C.c_void_p, "gsim_rowhash*": C.c_void_p, "gsim_rowhash**": C.POINTER(C.c_void_p),
             "gsim_rowset**": C.POINTER(C.c_void_p), "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "const uint32_t*": C.POINTER(C.c_uint32),
             "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64), "gsim_rowhash_stats*": C.POINTER(capi.GsimRowhashStats)}
    L = capi.load()
    for name in NEW:
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in proto.split(",")]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and [ctype[t] for t in types] == list(fn.argtypes), name


def test_the_header_states_the_hash_and_the_slot_rule_the_rule_restates():
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    for constant in ("0x9E3779B9", "0x85EBCA6B", "0xC2B2AE35", "0x2C1B3C6D", "0x297A2D39", "hash & (slots - 1)", "at least 1024"):
        assert constant in text, constant
    assert [R.slots(n) for n in (0, 1, 512, 513, 5000, 2 ** 31 + 1)] == [0, 1024, 1024, 2048, 16384, 2 ** 33]


@pytest.mark.parametrize("bits", WIDTHS)
def test_the_host_hash_is_the_rules_byte_for_byte(bits):
    rng = np.random.default_rng(bits)
    W = bits // 32
    single = np.zeros((min(bits, 96), W), np.uint32)
    for i, bit in enumerate(np.linspace(0, bits - 1, len(single)).astype(int)):
        single[i, bit // 32] = np.uint32(1 << (bit % 32))
    rows = np.concatenate([rng.integers(0, 2 ** 32, (200, W), dtype=np.uint32), np.zeros((1, W), np.uint32), np.full((1, W), 0xFFFFFFFF, np.uint32),
                           single])
    got = capi.row_hash(rows)
    assert got.dtype == np.uint64 and got.shape == (len(rows),)
    assert got.tobytes() == R.row_hash(rows).tobytes()
    assert len(set(got.tolist())) == len(got), "no two of these rows share a hash"
    assert len(capi.row_hash(np.zeros((0, W), np.uint32))) == 0
    if W >= 2:  # swapping two unequal words changes it
        for i in range(50):
            a, b = rng.choice(W, 2, replace=False)
            swapped = rows[i].copy()
            swapped[[a, b]] = swapped[[b, a]]
            assert rows[i, a] != rows[i, b] and capi.row_hash(swapped[None])[0] != got[i]
        zeros_but_one = np.zeros((2, W), np.uint32)
        zeros_but_one[0, 0] = zeros_but_one[1, W - 1] = 5
        h = capi.row_hash(zeros_but_one)
        assert h[0] != h[1]


def same_as_the_rule(rows):
    first, size, ngroups = capi.duplicates(rows)
    wfirst, wsize, counts = R.groups(rows)
    assert first.dtype == np.uint32 and size.dtype == np.uint32
    assert first.tobytes() == wfirst.tobytes() and size.tobytes() == wsize.tobytes() and ngroups == counts["groups"]
    return first, size, ngroups


@pytest.mark.parametrize("bits", [32, 160, 1024])
def test_duplicates_equal_the_rule(bits):
    rng = np.random.default_rng(0xD0 + bits)
    W = bits // 32
    for n in (0, 1, 2, 700, 3000):  # (700 rows: 2048 slots, 3000: 8192)
        rows = rng.integers(0, 2 ** 32, (n, W), dtype=np.uint32)
        if n >= 700:
            at = rng.permutation(n)
            rows[at[:300]] = rows[at[300]]
            rows[at[301:304]] = rows[at[304]]
            rows[at[305:400]] = rows[at[rng.integers(400, n, 95)]]
        same_as_the_rule(rows)
    _, size, g = same_as_the_rule(np.tile(rng.integers(0, 2 ** 32, (1, W), dtype=np.uint32), (500, 1)))
    assert g == 1 and (size == 500).all()
    _, size, g = same_as_the_rule(np.arange(600 * W, dtype=np.uint32).reshape(600, W))
    assert g == 600 and (size == 1).all()
    first, size, g = same_as_the_rule(np.zeros((40, W), np.uint32))
    assert g == 1 and (first == 0).all() and (size == 40).all(), "all-zero rows are an ordinary group"
    for word in (0, W - 1):  # rows that differ only in the first word, only in the last
        rows = np.tile(rng.integers(0, 2 ** 32, (1, W), dtype=np.uint32), (64, 1))
        rows[:, word] ^= np.uint32(1) << (np.arange(64, dtype=np.uint32) % np.uint32(32))
        first, size, g = same_as_the_rule(rows)
        assert g == 32 and (size == 2).all() and (first == np.arange(64) % 32).all()


def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "rowhash_front_errors.json")) as f:
        return json.load(f)


def test_every_front_case_answers_as_recorded():
    want = recorded()
    got = json.loads(json.dumps(cases.run_all()))
    assert sorted(got) == sorted(want), "the case list and the recorded file name the same cases"
    assert len(got) >= 55 and {c.split(":")[0] for c in got} == set(cases.ENTRIES)
    wrong = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not wrong, wrong


def test_the_recorded_file_holds_what_it_should():
    """Argument errors are INVALID with a message and come before any device state; a valid call of a device entry point is the state
    error of a table without rows on a GPU; the host functions and the calls that read the index alone are GSIM_OK."""
    want = recorded()
    for case, r in want.items():
        entry, what = case.split(": ", 1)
        if not what.startswith("valid"):
            assert r["code"] == INVALID and r["message"] and "GPU" not in r["message"], case
        elif entry in cases.ANSWERED:
            assert r["code"] == OK and r["message"] == "", case
        else:
            assert r["code"] == STATE and r["message"] == "table not finalized (no rows on a GPU)", case
            assert all(v in ("untouched", "cleared", None) for v in r["out"].values()), case
    for case in ("NULL db", "unknown flags", "valid", "a row base that takes the last row to GSIM_ROW_NONE"):
        assert want["rowhash_create: " + case]["out"]["out"] == "cleared", "*out is cleared on failure"
    assert want["rowhash_rowset: unknown flags"]["out"]["out"] == "cleared" and want["rowhash_rowset: valid"]["out"]["out"] == "cleared"
    assert want["rowhash_create: unknown flags"]["message"] == "unknown row-hash flags"
    assert want["rowhash_groups: both first and size NULL"]["message"] == "row hash: both first and size are NULL"
    assert want["rowhash_find_db: a left table of other fp_bits"]["message"] == "the two handles have different fp_bits"
    assert want["rowhash_find_db: a range past the left rows"]["message"] == "left row range outside the left table"
    h = np.array(want["row_hash: valid"]["out"]["hash"], np.uint32).view(np.uint64)
    assert h.tobytes() == R.row_hash(np.array([[1, 2], [2, 1]], np.uint32)).tobytes() and h[0] != h[1]
    d = want["duplicates: valid"]["out"]
    assert d["first"] == [0, 1, 0] and d["size"] == [2, 1, 2] and d["ngroups"] == [2, 0]


def test_python_wrappers_refuse_a_table_without_a_gpu():
    t = capi.Table(64).add_rows(np.arange(20, dtype=np.uint32).reshape(10, 2))
    with pytest.raises(capi.GsimError) as e:
        t.rowhash()
    assert e.value.code == STATE
    with pytest.raises(capi.GsimError) as e:
        capi.row_hash(np.zeros((2, 1025), np.uint32))
    assert e.value.code == INVALID
    t.close()


def test_the_stand_alone_checker_builds_plainly_and_under_the_sanitizers_and_passes():
    src = os.path.join(ROOT, "tests", "cpp", "rowhash_host_check.cpp")
    host = os.path.join(ROOT, "gpusimilarity_amd", "csrc", "capi_rowhash_host.cpp")
    deps = [src, host, os.path.join(ROOT, "gpusimilarity_amd", "csrc", "gsim_rowhash_hash.h"), os.path.join(ROOT, "include", "gpusim_hip.h")]
    common = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    for name, extra in (("rowhash_host_check", []),
                        ("rowhash_host_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exe = os.path.join(ROOT, "tests", "cpp", name)
        if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
            subprocess.check_call(common + extra + ["-o", exe, src, host])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], (name, r.stdout + r.stderr)
