"""Time gsim_db_neighbors phase by phase (HIP events inside the library: tile kernel, CSR build, D2H) on synthetic tables,
and report pairs/s against the VALU engine's ceiling.

    python scripts/time_neighbors.py [--rows 1000000] [--bits 1024] [--cutoff 0.7] [--kinds sparse,morgan] [--reps 2]

Ceiling: 8.8 cycles per wave64 word-pair instruction pair per SIMD (the scalar-operand v_and + v_bcnt of the r01 probe),
1024 SIMDs, 64 pairs per instruction pair, rows padded to WP words (4, 8, ... 128) -- reported at each clock of --mhz
(default: 2400 MHz peak and 2100 MHz) and at the clock the tile kernel itself measured (gsim_graph_stats.clock_mhz:
s_memtime cycles over the 100 MHz wall clock).  The upper triangle of an
N-row table is N (N - 1) / 2 pairs; pairs/s divides that by the tile-kernel time of the call."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

KINDS = {"sparse": capi.SYNTH_SPARSE, "dense": capi.SYNTH_DENSE, "morgan": capi.SYNTH_MORGAN}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--cutoff", type=float, default=0.7)
    ap.add_argument("--kinds", default="sparse,morgan")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--mhz", type=float, nargs="*", default=[2400.0, 2100.0])
    ap.add_argument("--json", default=None)
    ap.add_argument("--identical", action="store_true",
                    help="worst case of the emission: every row the same (every pair kept), rows uploaded from the host")
    a = ap.parse_args()
    W = a.bits // 32
    wp = 4
    while wp < W:
        wp *= 2
    n = a.rows
    pairs = n * (n - 1) / 2
    out = []
    for kind in a.kinds.split(","):
        if a.identical:
            row = capi.synth_row(0xC0FFEE, KINDS[kind], 0, a.bits)
            t = capi.Table(a.bits).add_rows(np.tile(row, (n, 1))).finalize(0, 1)
        else:
            t = capi.Table(a.bits).generate(0xC0FFEE, KINDS[kind], 0, n, 0)
        t.neighbors(a.cutoff)  # warm-up: sizes the pair buffer, loads the kernels
        for rep in range(a.reps):
            st = {}
            w0 = time.perf_counter()
            indptr, indices, scores = t.neighbors(a.cutoff, stats=st)
            wall = time.perf_counter() - w0
            rec = dict(kind=kind, rows=n, bits=a.bits, cutoff=a.cutoff, rep=rep, nnz=int(len(indices)), pairs=int(st["pairs"]),
                       launches=int(st["launches"]), launches_rerun=int(st["launches_rerun"]), tile_ms=st["tile_ms"],
                       csr_ms=st["csr_ms"], d2h_ms=st["d2h_ms"], call_ms=st["wall_ms"], python_wall_ms=wall * 1e3,
                       pairs_per_s=pairs / (st["tile_ms"] * 1e-3), whole_over_tile=st["wall_ms"] / st["tile_ms"])
            rec["clock_mhz_measured"] = st["clock_mhz"]
            for mhz in list(a.mhz) + [st["clock_mhz"]]:
                ceil = 1024 * mhz * 1e6 / 8.8 * 64 / wp  # pairs/s at wp words per row
                rec["ceiling_pairs_per_s@%dMHz" % round(mhz)] = ceil
                rec["fraction_of_ceiling@%dMHz" % round(mhz)] = rec["pairs_per_s"] / ceil
            print(json.dumps(rec), flush=True)
            out.append(rec)
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
