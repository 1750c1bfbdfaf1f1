"""Time gsim_db_maxmin on synthetic tables and report the per-pick cost against HBM.

    python scripts/time_maxmin.py [--rows 1000000 100000000] [--bits 1024] [--picks 1000] [--kinds sparse,morgan] [--reps 2]

Per pick: kernel_ms / picks (HIP events around all pass launches) and wall_ms / picks (the whole call).  Byte accounting of
one pass: N x (row bytes + 4) read (the table and maxsim), plus 8 B stored for every row whose maxsim rose (rows_updated: maxsim
and nearest); the fraction is those bytes over kernel_ms against 8 TB/s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpusimilarity_amd import capi  # noqa: E402

KINDS = {"sparse": capi.SYNTH_SPARSE, "dense": capi.SYNTH_DENSE, "morgan": capi.SYNTH_MORGAN}
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 100_000_000])
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--picks", type=int, default=1000)
    ap.add_argument("--kinds", default="sparse,morgan")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--assign", action="store_true", help="also return row_score / nearest (the nearest store on)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = []
    for n in a.rows:
        for kind in a.kinds.split(","):
            t = capi.Table(a.bits).generate(0xC0FFEE, KINDS[kind], 0, n, 0)
            t.maxmin(min(8, n))  # warm-up: loads the kernels
            for rep in range(a.reps):
                st = {}
                w0 = time.perf_counter()
                t.maxmin(a.picks, assign=a.assign, stats=st)
                wall = time.perf_counter() - w0
                picks = int(st["picks"])
                passes = picks if a.assign else picks - 1
                nbytes = passes * n * (a.bits // 8 + 4) + st["rows_updated"] * (8 if a.assign else 4)
                rec = dict(kind=kind, rows=n, bits=a.bits, picks=picks, assign=a.assign, rep=rep, launches=int(st["launches"]),
                           rows_updated=int(st["rows_updated"]), kernel_ms=st["kernel_ms"], d2h_ms=st["d2h_ms"],
                           call_ms=st["wall_ms"], python_wall_ms=wall * 1e3,
                           kernel_ms_per_pick=st["kernel_ms"] / picks, wall_ms_per_pick=st["wall_ms"] / picks,
                           bytes=nbytes, fraction_of_8TBps=nbytes / (st["kernel_ms"] * 1e-3) / PEAK)
                print(json.dumps(rec), flush=True)
                out.append(rec)
            t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
