"""Time gsim_db_linkage (the library's own clocks: the matrix pass, the chain launches, the host's replay) on Morgan-shaped synthetic
rows, both linkages, beside gsim_db_mst on the same rows in the same run.

    python scripts/time_linkage.py [--rows 4096,16384,65536] [--bits 1024] [--reps 2] [--launch-steps 0] [--out profiles/linkage_time.txt]

Per call: matrix ms, chain ms, scans, the chain's microseconds and GB/s per scan -- a scan reads one matrix row (4 or 8 bytes an entry)
and the cluster sizes (4 bytes an entry) -- beside the range the per-CU gather rates give one compute unit: 23 GB/s (rows streamed
from HBM) to 73 GB/s (rows served by the L2).  The chain's time also holds its merges (two rows read, one row and one column
written each), so the rate per scan is a lower bound."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

TINY = float(np.nextafter(np.float32(0), np.float32(1)))
PER_CU_GBS = (23.0, 73.0)
NAMES = {capi.LINKAGE_COMPLETE: "complete", capi.LINKAGE_AVERAGE: "average"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--launch-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkage_time.txt"))
    a = ap.parse_args()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        with open(a.out, "w") as f:  # (kept as far as the run got)
            f.write("\n".join(lines) + "\n")

    for rows in [int(r) for r in a.rows.split(",")]:
        what = "morgan %d x %d" % (rows, a.bits)
        t = capi.Table(a.bits).generate(0xC0FFEE, capi.SYNTH_MORGAN, 0, rows, 0)
        t.linkage(capi.LINKAGE_COMPLETE, 0, min(rows, 512))  # warm-up: loads the kernels
        for kind in (capi.LINKAGE_COMPLETE, capi.LINKAGE_AVERAGE):
            for rep in range(a.reps):
                try:
                    m, st = t.linkage(kind, launch_steps=a.launch_steps)
                except capi.GsimError as e:
                    emit(call="linkage", table=what, linkage=NAMES[kind], rep=rep, error=str(e))
                    break
                row_bytes = rows * ((8 if kind == capi.LINKAGE_AVERAGE else 4) + 4)
                us = st["chain_ms"] * 1e3 / st["scans"]
                emit(call="linkage", table=what, linkage=NAMES[kind], rep=rep, matrix_ms=st["matrix_ms"], chain_ms=st["chain_ms"],
                     order_ms=st["order_ms"], d2h_ms=st["d2h_ms"], wall_ms=st["wall_ms"], scans=int(st["scans"]),
                     chain_max=int(st["chain_max"]), launches=int(st["launches"]), launch_steps=int(st["launch_steps"]),
                     ms_per_launch=st["chain_ms"] / st["launches"], clock_mhz=st["clock_mhz"], bytes_per_scan=row_bytes, us_per_scan=us,
                     gb_per_s_per_scan=row_bytes / us * 1e-3, per_cu_gb_per_s=PER_CU_GBS, top_score=float(m["score"][0]),
                     last_score=float(m["score"][-1]), distinct_scores=int(len(np.unique(m["score"]))))
        for rep in range(a.reps):
            edges, st = t.mst(TINY)
            emit(call="mst", table=what, cutoff=TINY, rep=rep, edges=int(len(edges)), rounds=int(st["rounds"]), kernel_ms=st["kernel_ms"],
                 wall_ms=st["wall_ms"])
        t.close()


if __name__ == "__main__":
    main()
