"""Time gsim_db_search_group on generated Morgan-shaped tables.

    python scripts/time_group.py [--rows 1000000,100000000] [--bits 1024] [--k 1000] [--sizes 1,4,16,64,256] [--reps 3]
                                 [--timeout 300] [--out FILE.json]

For every table size N and every query-set size M, one child process (its own `timeout`; the script stops at the first one that
fails or runs out of time) generates the table and reports, for MAX, MIN and MEAN:
  scan_ms / kernel_ms / wall_ms   best of --reps calls (HIP events inside the library: the scan launches, scan + tail; host clock)
  launches                        kernel launches of the call (GSIM_GROUP_LAUNCH_PAIRS, or the default by row width, cuts the pass)
  launch_ms                       scan_ms / the scan's launches (the call's less the tail's three, k <= 8192): what has to stay short
  pairs_per_s                     N x M / scan_ms
  valu_fraction                   pairs_per_s over the VALU ceiling of this loop form (v_and with a scalar operand +
                                  v_bcnt = 8 cycles per word pair per wave): CUs x 4 SIMDs x 64 rows x clock / (8 x words per row)
and beside them, in the same process on the same table, the same M queries as
  each_ms                         M single queries, gsim_db_search_each (the whole call, host clock)
  batch_ms                        one gsim_db_search call (a batch from 4 queries on)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x6A00
MODES = ["max", "min", "mean"]


def best_of(reps, fn):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def child(a):
    import numpy as np

    from gpusimilarity_amd import capi
    n, M, bits, k = a.child_rows, a.child_m, a.bits, a.k
    W = bits // 32
    t = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, n, 0)
    queries = np.stack([capi.synth_row(SEED, capi.SYNTH_MORGAN, n + i, bits) for i in range(M)])
    ceiling = a.cus * 4 * 64 * a.mhz * 1e6 / (8.0 * W)
    bufs = t.make_search_buffers(M, k)
    t.search_each_into(queries, k, bufs)  # warm-up: loads the kernels, allocates the scratch
    each_ms = best_of(a.reps, lambda: t.search_each_into(queries, k, bufs))
    t.search_into(queries, k, bufs)
    batch_ms = best_of(a.reps, lambda: t.search_into(queries, k, bufs))
    for mode, name in enumerate(MODES):
        t.search_group(queries, k, mode)
        best = None
        for _ in range(a.reps):
            _, _, st = t.search_group(queries, k, mode, stats=True)
            if best is None or st["scan_ms"] < best["scan_ms"]:
                best = st
        pairs_per_s = best["pairs"] / (best["scan_ms"] * 1e-3)
        launch_ms = best["scan_ms"] / max(best["launches"] - 3, 1) if k <= capi.SELECT_CAP else None
        print(json.dumps(dict(rows=n, bits=bits, k=k, M=M, mode=name, launches=best["launches"], launch_ms=launch_ms, scan_ms=best["scan_ms"],
                              kernel_ms=best["kernel_ms"], wall_ms=best["wall_ms"], pairs_per_s=pairs_per_s,
                              valu_fraction=pairs_per_s / ceiling, each_ms=each_ms, batch_ms=batch_ms)), flush=True)
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,100000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--sizes", default="1,4,16,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cus", type=int, default=256, help="compute units (the VALU ceiling)")
    ap.add_argument("--mhz", type=float, default=2400.0, help="engine clock (the VALU ceiling)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-rows", type=int, default=0)
    ap.add_argument("--child-m", type=int, default=0)
    a = ap.parse_args()
    if a.child_rows:
        return child(a)
    sink = []
    rc = 0
    for n in (int(x) for x in a.rows.split(",")):
        for M in (int(x) for x in a.sizes.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--child-rows", str(n), "--child-m", str(M), "--bits", str(a.bits), "--k", str(a.k),
                   "--reps", str(a.reps), "--cus", str(a.cus), "--mhz", str(a.mhz)]
            try:
                out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True).stdout.decode()
            except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as e:
                print("stopping: rows %d, M %d: %s" % (n, M, e), file=sys.stderr)
                rc = 1
                break
            for line in out.splitlines():
                if line.startswith("{"):
                    print(line, flush=True)
                    sink.append(json.loads(line))
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            json.dump(sink, f, indent=1)
            f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
