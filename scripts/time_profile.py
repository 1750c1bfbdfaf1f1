"""Time gsim_db_bit_counts and gsim_db_overlap_sums (HIP events inside the library around the pass) beside gsim_db_search on the same
table in the same run, and report ms, rows/s and the fraction of 8 TB/s of every pass.

    python scripts/time_profile.py [--rows 1000000,100000000] [--bits 1024,160] [--kinds sparse,dense,morgan] [--reps 3]
                                   [--out profiles/profile_time.txt]

Per table: one gsim_db_search (k = 100, host clock around the call, the best of the repetitions), the column counts of the whole table,
the overlap sums with the table's own counts as weights (as many bit planes as the row count has bits) and with full 32-bit weights.
At the largest row count of 1024-bit rows also a 1 % and a 50 % row set, each on both routes (GSIM_SUBSET_GATHER_MAX_PERMILLE 0 and
1000 on two handles).  Where the test-hooks build of the library is present, a child process repeats the overlap sums with the VALU
kernel forced (GSIM_TEST_PROFILE_VALU = 1) on the widths the matrix cores take otherwise: the two routes side by side.
Bytes: rows read x row bytes; the outputs (8 or 12 bytes per row of gsim_db_overlap_sums) are not counted."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

KINDS = {"sparse": capi.SYNTH_SPARSE, "dense": capi.SYNTH_DENSE, "morgan": capi.SYNTH_MORGAN}
ROUTES = {capi.PROFILE_STREAMED: "streamed", capi.PROFILE_GATHERED: "gathered", capi.PROFILE_MATRIX: "matrix", capi.PROFILE_VALU: "valu"}
HBM = 8e12
HOOKS_LIB = os.path.join(ROOT, "gpusimilarity_amd", "testhooks", "libgsim_hip.so")
SEED = 0xC0FFEE


def route_name(bits):
    return "+".join(name for bit, name in ROUTES.items() if int(bits) & bit)


def make(bits, kind, rows, gather=None):
    old = os.environ.get("GSIM_SUBSET_GATHER_MAX_PERMILLE")
    if gather is not None:
        os.environ["GSIM_SUBSET_GATHER_MAX_PERMILLE"] = gather
    try:
        return capi.Table(bits).generate(SEED, KINDS[kind], 0, rows, 0)
    finally:
        if gather is not None:
            if old is None:
                os.environ.pop("GSIM_SUBSET_GATHER_MAX_PERMILLE", None)
            else:
                os.environ["GSIM_SUBSET_GATHER_MAX_PERMILLE"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,100000000")
    ap.add_argument("--bits", default="1024,160")
    ap.add_argument("--kinds", default="sparse,dense,morgan")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_time.txt"))
    ap.add_argument("--valu-child", action="store_true", help="(internal) only the overlap sums, printed, nothing written")
    a = ap.parse_args()
    all_rows = [int(r) for r in a.rows.split(",")]
    all_bits = [int(b) for b in a.bits.split(",")]
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def report(call, what, st, row_bytes, **more):
        ms = st["kernel_ms"]
        emit(call=call, table=what, route=route_name(st["route"]), kernel_ms=ms, d2h_ms=st["d2h_ms"], wall_ms=st["wall_ms"],
             launches=int(st["launches"]), rows_read=int(st["rows_read"]), rows_counted=int(st["rows_counted"]),
             rows_per_s=st["rows_read"] / (ms * 1e-3) if ms else None,
             fraction_of_8TBs=st["rows_read"] * row_bytes / (ms * 1e-3) / HBM if ms else None, **more)

    def best_of(call):
        best = None
        for rep in range(a.reps + 1):  # (the first is the warm-up)
            st = {}
            call(st)
            if rep and (best is None or st["kernel_ms"] < best["kernel_ms"]):
                best = st
        return best

    for bits in all_bits:
        row_bytes = bits // 8
        for rows in all_rows:
            for kind in a.kinds.split(","):
                what = "%s %d x %d" % (kind, rows, bits)
                t = make(bits, kind, rows)
                counts, counted = t.bit_counts()
                assert counted == rows
                full = np.random.default_rng(bits).integers(2**31, 2**32, bits, dtype=np.uint64)
                if not a.valu_child:
                    q = capi.synth_row(SEED, KINDS[kind], rows // 2, bits)
                    ms = []
                    for rep in range(a.reps + 1):
                        t0 = time.perf_counter()
                        t.search(q, 100)
                        ms.append((time.perf_counter() - t0) * 1e3)
                    emit(call="search", table=what, k=100, wall_ms=min(ms[1:]), rows_per_s=rows / (min(ms[1:]) * 1e-3),
                         fraction_of_8TBs=rows * row_bytes / (min(ms[1:]) * 1e-3) / HBM)
                    report("bit_counts", what, best_of(lambda st: t.bit_counts(stats=st)), row_bytes, search_wall_ms=min(ms[1:]))
                tag = dict(forced="valu") if a.valu_child else {}
                report("overlap_sums", what, best_of(lambda st: t.overlap_sums(counts, stats=st)), row_bytes,
                       weights="counts", planes=int(counts.max()).bit_length(), **tag)
                report("overlap_sums", what, best_of(lambda st: t.overlap_sums(full, popc=True, stats=st)), row_bytes,
                       weights="32-bit", planes=32, popc=True, **tag)
                t.close()
        # both row-set routes at the largest table of this width
        if a.valu_child or bits != 1024:
            continue
        rows = max(all_rows)
        rng = np.random.default_rng(1)
        one = np.unique(np.arange(0, rows, 100, dtype=np.int64) + rng.integers(0, 100, (rows + 99) // 100)).astype(np.uint32)
        one = one[one < rows]
        half = rng.integers(0, 2**32, (rows + 31) // 32, dtype=np.uint64).astype(np.uint32)
        for gather, name in (("0", "streamed"), ("1000", "gathered")):
            t = make(bits, "morgan", rows, gather)
            what = "morgan %d x %d" % (rows, bits)
            for share, kw in (("1 %", dict(rows=one)), ("50 %", dict(bitmap=half))):
                rs = t.rowset(**kw)
                st = best_of(lambda st: t.bit_counts(rs, stats=st))
                assert route_name(st["route"]) == name
                report("bit_counts", what, st, row_bytes, rowset=share, selected=int(rs.count))
                rs.close()
            t.close()
    if a.valu_child:
        return
    if os.path.exists(HOOKS_LIB):
        wide = [b for b in all_bits if b % 256 == 0]
        if wide:
            env = dict(os.environ, GSIM_LIB=HOOKS_LIB, GSIM_TEST_PROFILE_VALU="1")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--valu-child", "--rows", a.rows, "--bits", ",".join(map(str, wide)),
                                "--kinds", a.kinds, "--reps", str(a.reps)], env=env, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("the VALU child failed:\n" + r.stdout[-2000:] + r.stderr[-3000:])
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    lines.append(line)
                    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
