"""The tuning knobs (gpusimilarity_amd/csrc/capi_knobs.h): which names the shipped library reads, and what read_knobs() makes of a string.

The names: the NUL-delimited strings of libgsim_hip.so that are a GSIM_[A-Z0-9_]+ name and nothing else are the literal list below and
the names in the first column of INTEGRATION.md's knob table; no retired name and no GSIM_TEST_* hook is among them.

The parsing: tests/cpp/knobs_check.cpp links the knobs' translation unit, sets one variable at a time and compares the knob with
tests/golden/knobs_parse.tsv -- every knob unset, empty, "0", "1", negative, garbage, around each clamp and beyond int and long long.
The table was recorded once from the hand-written read_knobs() of commit 86472ac, the last before the reader became a table: a
program that included that commit's capi_internal.h and linked its libgsim_hip.so set each string, called read_knobs() and printed the
member.  It is a record of that reader: a new knob gets new lines (the checker refuses a knob without any), existing lines stay."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "gpusimilarity_amd")

KNOBS = """GSIM_FUSED GSIM_FUSED_DEBUG GSIM_FUSED_FLAGS GSIM_FUSED_SELECT_MAX_K GSIM_FUSED_BACKOFF GSIM_PUBLISH_MIN_ROWS_PER_K
GSIM_LARGEK_BINRANK GSIM_LARGEK_ONE_BLOCK_MAX GSIM_EACH_LANES
GSIM_BATCH_MFMA_MIN_Q GSIM_BATCH_MFMA_DENSE GSIM_BATCH_SEG_CAP_INIT GSIM_BATCH_SEG_CAP GSIM_DEBUG_BATCH GSIM_FOLD_RESCORE
GSIM_JOIN_STREAM_MAX_ROWS GSIM_SUBSET_GATHER_MAX_PERMILLE GSIM_GROUP_LAUNCH_PAIRS GSIM_LEADER_ROUND GSIM_LEADER_LAUNCH_PAIRS
GSIM_KNN_LAUNCH_PAIRS GSIM_KNN_JOIN_SEGMENTS GSIM_KNN_JOIN_LAUNCH_PAIRS GSIM_HIST_STREAM_MAX_ROWS GSIM_HIST_LAUNCH_PAIRS GSIM_HIST_NAIVE_ADD
GSIM_SCORES_LAUNCH_PAIRS GSIM_SCORES_STAGE_BYTES GSIM_COMPONENTS_LAUNCH_PAIRS GSIM_MST_LAUNCH_PAIRS GSIM_DBSCAN_LAUNCH_PAIRS GSIM_DBSCAN_SKIP
GSIM_PROFILE_LAUNCH_ROWS GSIM_ASSIGN_LAUNCH_PAIRS GSIM_LABELS_LAUNCH_ROWS""".split()

RETIRED = """GSIM_SCAN_WAVES_PER_CU GSIM_SCAN_RAGGED GSIM_SAMPLE_CHUNKS GSIM_SAMPLE_SHIFT GSIM_FUSED_MAX_ROWS GSIM_FUSED_SEED_NARROW
GSIM_FUSED_PUBLISH GSIM_FUSED_PUBLISH_MAX_K GSIM_PUBLISH_NARROW GSIM_LARGEK_BINRANK_MAX_K GSIM_EACH_PIPELINE GSIM_EACH_LANES_SHARE
GSIM_EACH_LANES_PUBLISH GSIM_EACH_LANES_MAX_MB GSIM_BATCH GSIM_BATCH_WAVES_PER_CU GSIM_BATCH_SAMPLE_CHUNKS GSIM_BATCH_RPL
GSIM_BATCH_MFMA_SAMPLE GSIM_FOLD_FULL_ON_DEVICE""".split()


def library_strings():
    data = open(os.path.join(LIBDIR, "libgsim_hip.so"), "rb").read()
    return data, {m.group(1).decode() for m in re.finditer(rb"\0(GSIM_[A-Z0-9_]+)(?=\0)", data)}


def test_the_shipped_library_reads_exactly_the_listed_names():
    assert len(KNOBS) == len(set(KNOBS)) == 35 and len(RETIRED) == len(set(RETIRED)) == 20 and not set(KNOBS) & set(RETIRED)
    data, names = library_strings()
    assert names == set(KNOBS), (sorted(names - set(KNOBS)), sorted(set(KNOBS) - names))
    assert not [n for n in names if n.startswith("GSIM_TEST_")] and b"GSIM_TEST" not in data
    assert not names & set(RETIRED)


def test_the_knob_table_of_the_integration_guide_lists_the_same_names():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("| knob (default) | effect |"):]
    rows = [l for l in table.splitlines()[2:]]
    rows = rows[:next(i for i, l in enumerate(rows) if not l.lstrip().startswith("|"))]
    listed = [n for l in rows for n in re.findall(r"`(GSIM_[A-Z0-9_]+)`", l.split("|")[1])]
    assert len(listed) == len(set(listed)), "a knob has one row"
    assert set(listed) == set(KNOBS), (sorted(set(listed) - set(KNOBS)), sorted(set(KNOBS) - set(listed)))


def test_read_knobs_gives_the_recorded_value_for_every_string():
    src = os.path.join(ROOT, "tests", "cpp", "knobs_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "knobs_check")
    csrc = os.path.join(LIBDIR, "csrc")
    unit = os.path.join(csrc, "capi_knobs.cpp")
    gold = os.path.join(ROOT, "tests", "golden", "knobs_parse.tsv")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    deps = [src, unit, os.path.join(csrc, "capi_knobs.h"), os.path.join(csrc, "gsim_device.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-o", exe, src, unit])
    lines = [l.split("\t") for l in open(gold).read().splitlines() if l and not l.startswith("#")]
    assert {l[0] for l in lines} == set(KNOBS)
    for name in KNOBS:  # what the issue asks of every knob: unset, "", "0", "1", a negative, garbage, and the far side of int and long long
        have = {(l[1], l[2]) for l in lines if l[0] == name}
        assert {("unset", ""), ("set", ""), ("set", "0"), ("set", "1"), ("set", "-5"), ("set", "abc"), ("set", "2147483648"),
                ("set", "-2147483649"), ("set", "99999999999"), ("set", "-99999999999")} <= have, name
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSIM_")}
    r = subprocess.run([exe, gold], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout[-3000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[1]) == len(lines)
