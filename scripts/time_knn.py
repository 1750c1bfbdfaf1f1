"""Time gsim_db_knn (HIP events inside the library: the fold kernel's launches, the CSR build, D2H) on synthetic tables made on the
device, beside two yardsticks on the same table in the same run, and report pairs/s against the VALU engine's ceiling (DESIGN.md
section 9) at the clock the fold kernel itself measured.

    python scripts/time_knn.py [--rows 1000000] [--bits 1024] [--kinds morgan,sparse] [--ks 8,32,128] [--owners 0]

Per table, k and cutoff (the smallest positive float, and 0.5): kernel ms, launches, the mean launch, inserts (per owner row too),
pairs/s, the fraction of the ceiling, and the ratios to the yardsticks:
  (a) gsim_db_neighbors on a row range of the same table (a rectangle: no triangle saving) at cutoff 0.7 -- the same engine without
      lists; its pair rate is what the fold kernel's is compared with;
  (b) the only route to these lists without gsim_db_knn: gsim_db_search with 256 of the table's own rows per call at k + 1, over
      4096 owner rows, scaled to the table (ms per owner row x rows).
--owners R > 0 folds only the owner rows [0, R) (pairs = R x rows), for a quick look.
Ceiling: 8.8 cycles per wave64 word-pair instruction pair per SIMD, 1024 SIMDs, 64 pairs per instruction pair, rows padded to WP
words (scripts/time_neighbors.py).  The stats carry no per-launch times: the longest launch is not reported, the mean is."""
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
TINY = float(np.nextafter(np.float32(0), np.float32(1)))
SEED = 0xC0FFEE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--kinds", default="morgan,sparse")
    ap.add_argument("--ks", default="8,32,128")
    ap.add_argument("--owners", type=int, default=0, help="fold only the owner rows [0, OWNERS) (0: the whole table)")
    ap.add_argument("--nbr-rows", type=int, default=131072, help="rows of yardstick (a)'s rectangle")
    ap.add_argument("--search-rows", type=int, default=4096, help="owner rows of yardstick (b)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W = a.bits // 32
    wp = 4
    while wp < W:
        wp *= 2
    n = a.rows
    owners = a.owners if a.owners > 0 else n
    out = []
    for kind in a.kinds.split(","):
        t = capi.Table(a.bits).generate(SEED, KINDS[kind], 0, n, 0)
        # (a) the tile kernel on a rectangle of the same table
        nb = min(a.nbr_rows, n)
        t.neighbors(0.7, row_begin=0, row_end=min(nb, 4096))  # warm-up: sizes the pair buffer, loads the kernels
        st = {}
        t.neighbors(0.7, row_begin=0, row_end=nb, stats=st)
        nbr_rate = nb * n / (st["tile_ms"] * 1e-3)
        rec = dict(what="neighbors_rectangle", kind=kind, rows=n, bits=a.bits, left_rows=nb, cutoff=0.7, tile_ms=st["tile_ms"],
                   launches=int(st["launches"]), launches_rerun=int(st["launches_rerun"]), pairs_listed=int(st["pairs"]),
                   clock_mhz=st["clock_mhz"], pairs_per_s=nbr_rate,
                   fraction_of_ceiling=nbr_rate / (1024 * st["clock_mhz"] * 1e6 / 8.8 * 64 / wp))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        sr = min(a.search_rows, n)
        q = np.stack([capi.synth_row(SEED, KINDS[kind], r, a.bits) for r in range(sr)])
        for k in [int(x) for x in a.ks.split(",")]:
            for cutoff in (TINY, 0.5):
                # (b) 256 of the table's own rows per gsim_db_search call at k + 1
                t.search(q[:256], k + 1, cutoff)
                w0 = time.perf_counter()
                for lo in range(0, sr, 256):
                    t.search(q[lo:lo + 256], k + 1, cutoff)
                search_ms_per_row = (time.perf_counter() - w0) * 1e3 / sr
                t.knn(k, cutoff, row_begin=0, row_end=min(owners, 1024))  # warm-up
                st = {}
                indptr, indices, scores = t.knn(k, cutoff, row_begin=0, row_end=owners, stats=st)
                rate = st["pairs"] / (st["kernel_ms"] * 1e-3)
                ceil = 1024 * st["clock_mhz"] * 1e6 / 8.8 * 64 / wp
                rec = dict(what="knn", kind=kind, rows=n, bits=a.bits, owners=owners, k=k, cutoff=cutoff, kernel_ms=st["kernel_ms"],
                           launches=int(st["launches"]), mean_launch_ms=st["kernel_ms"] / max(st["launches"], 1), inserts=int(st["inserts"]),
                           inserts_per_owner=st["inserts"] / owners, entries=int(st["entries"]), csr_ms=st["csr_ms"],
                           d2h_ms=st["d2h_ms"], call_ms=st["wall_ms"], clock_mhz=st["clock_mhz"], pairs_per_s=rate,
                           fraction_of_ceiling=rate / ceil, rate_over_neighbors=rate / nbr_rate,
                           knn_ms_per_owner=st["wall_ms"] / owners, search_ms_per_owner=search_ms_per_row,
                           search_route_scaled_s=search_ms_per_row * n * 1e-3, knn_scaled_s=st["wall_ms"] / owners * n * 1e-3,
                           search_over_knn=search_ms_per_row / (st["wall_ms"] / owners))
                print(json.dumps(rec), flush=True)
                out.append(rec)
                del indptr, indices, scores
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
