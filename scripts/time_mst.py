"""Time gsim_db_mst (HIP events inside the library: the fold launches of every scan, the rounds' bookkeeping, the sort, D2H) on
synthetic tables, beside gsim_db_knn at k = 1 and one gsim_db_components pass on the same table in the same run, and report every
scan's pairs/s against the VALU engine's ceiling (DESIGN.md sections 9 and 19).

    python scripts/time_mst.py [--rows 100000,1000000] [--bits 1024] [--kinds sparse,morgan] [--reps 2] [--out profiles/mst_time.txt]

Per table: gsim_db_mst at the smallest positive cutoff and at 0.5; per scan its owner rows, kernel ms, pairs/s and fraction of the
ceiling.  Ceiling: as scripts/time_knn.py -- 8.8 cycles per wave64 v_and + v_bcnt pair per SIMD, 1024 SIMDs, 64 pairs per instruction
pair, rows padded to WP words -- at the clock the fold kernel itself measured (clock_mhz).  The rates count every owner x candidate pair
of a scan, also those the kernel skips because the wave's owners and the candidate are one component: above 1.0 is possible."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

KINDS = {"sparse": capi.SYNTH_SPARSE, "dense": capi.SYNTH_DENSE, "morgan": capi.SYNTH_MORGAN}
TINY = float(np.nextafter(np.float32(0), np.float32(1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--kinds", default="sparse,morgan")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mst_time.txt"))
    a = ap.parse_args()
    wp = 4
    while wp < a.bits // 32:
        wp *= 2
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def ceiling(mhz):
        return 1024 * mhz * 1e6 / 8.8 * 64 / wp  # pairs/s at wp words per row

    for rows in [int(r) for r in a.rows.split(",")]:
        for kind in a.kinds.split(","):
            what = "%s %d x %d" % (kind, rows, a.bits)
            t = capi.Table(a.bits).generate(0xC0FFEE, KINDS[kind], 0, rows, 0)
            t.knn(1, TINY, row_end=min(rows, 4096))  # warm-up: loads the kernels
            knn_ms = []
            for rep in range(a.reps):
                st = {}
                t.knn(1, TINY, stats=st)
                knn_ms.append(st["kernel_ms"])
                emit(call="knn", table=what, k=1, cutoff=TINY, rep=rep, kernel_ms=st["kernel_ms"], wall_ms=st["wall_ms"],
                     launches=int(st["launches"]), clock_mhz=st["clock_mhz"],
                     fraction_of_ceiling=rows * rows / (st["kernel_ms"] * 1e-3) / ceiling(st["clock_mhz"]) if st["clock_mhz"] else None)
            comp_ms = {}
            for cutoff in (TINY, 0.5):
                t.components(cutoff, first_row=False, sizes=False)  # warm-up
                levels, st = t.components(cutoff)
                comp_ms[cutoff] = st["wall_ms"]
                emit(call="components", table=what, cutoff=cutoff, kernel_ms=st["kernel_ms"], wall_ms=st["wall_ms"],
                     ncomponents=int(len(levels[0][1])), largest=int(levels[0][2].max()))
            for cutoff in (TINY, 0.5):
                best = None
                for rep in range(a.reps + 1):  # (the first is the warm-up)
                    edges, st = t.mst(cutoff)
                    if rep == 0:
                        continue
                    mhz = st["clock_mhz"]
                    scans = [dict(owners=int(o), kernel_ms=ms, pairs_per_s=o * rows / (ms * 1e-3) if ms else None,
                                  fraction_of_ceiling=o * rows / (ms * 1e-3) / ceiling(mhz) if ms and mhz else None)
                             for o, ms in zip(st["scan_owners"], st["scan_kernel_ms"])]
                    emit(call="mst", table=what, cutoff=cutoff, rep=rep - 1, rounds=int(st["rounds"]), scans=scans, edges=int(st["edges"]),
                         launches=int(st["launches"]), owner_rows=int(st["owner_rows"]), kernel_ms=st["kernel_ms"], round_ms=st["round_ms"],
                         sort_ms=st["sort_ms"], d2h_ms=st["d2h_ms"], wall_ms=st["wall_ms"], clock_mhz=mhz)
                    if best is None or st["wall_ms"] < best["wall_ms"]:
                        best = st
                first = best["scan_kernel_ms"][0]
                emit(summary=what, cutoff=cutoff, rounds=int(best["rounds"]), scan1_kernel_ms=first, knn_k1_kernel_ms=min(knn_ms),
                     scan1_over_knn=first / min(knn_ms), mst_wall_ms=best["wall_ms"], components_wall_ms=comp_ms[cutoff],
                     mst_over_components=best["wall_ms"] / comp_ms[cutoff], bar_passes=2 * int(best["rounds"]))
            t.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
