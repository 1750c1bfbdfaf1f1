"""Time gsim_db_mreach_mst (HIP events inside the library: the core pass's fold launches and tail kernel, the fold launches of every
scan, the rounds' bookkeeping, the sort, D2H) on synthetic tables, beside gsim_db_knn at k = min_pts - 1 and gsim_db_mst on the same
table at the same cutoff in the same run, and the host selection gsim_mst_hdbscan on the forest (DESIGN.md sections 19 and 28).

    python scripts/time_hdbscan.py [--rows 100000,1000000] [--bits 1024] [--kinds morgan] [--min-pts 5,16] [--reps 1]
                                   [--out profiles/hdbscan_time.txt]

Per table and cutoff (the smallest positive float, and 0.5): gsim_db_mst's scans; then per min_pts the k-NN fold, the forest's core
pass and scans -- per scan its owner rows, kernel ms, pairs/s and fraction of the VALU ceiling -- and the selection's host ms at
min_cluster_size = min_pts.  Ceiling: as scripts/time_mst.py -- 8.8 cycles per wave64 v_and + v_bcnt pair per SIMD, 1024 SIMDs, 64
pairs per instruction pair, rows padded to WP words -- at the clock the fold kernel itself measured.  The rates count every owner x
candidate pair of a scan, also those the kernel skips before it reads the candidate: above 1.0 is possible.  The summary lines hold
the two ratios of section 28: scan 1 over gsim_db_mst's scan 1, and the core pass's fold over gsim_db_knn's."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--kinds", default="morgan")
    ap.add_argument("--min-pts", default="5,16")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_time.txt"))
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

    def scans_of(st, rows):
        mhz = st["clock_mhz"]
        return [dict(owners=int(o), kernel_ms=ms, pairs_per_s=o * rows / (ms * 1e-3) if ms else None,
                     fraction_of_ceiling=o * rows / (ms * 1e-3) / ceiling(mhz) if ms and mhz else None)
                for o, ms in zip(st["scan_owners"], st["scan_kernel_ms"])]

    min_pts = [int(m) for m in a.min_pts.split(",")]
    # warm-up on a small table: loads every kernel the timed calls use
    w = capi.Table(a.bits).generate(0xC0FFEE, KINDS[a.kinds.split(",")[0]], 0, 4096, 0)
    for mp in min_pts:
        w.knn(mp - 1, TINY)
        w.mreach_mst(mp, TINY)
    w.mst(TINY)
    w.close()
    for rows in [int(r) for r in a.rows.split(",")]:
        for kind in a.kinds.split(","):
            what = "%s %d x %d" % (kind, rows, a.bits)
            t = capi.Table(a.bits).generate(0xC0FFEE, KINDS[kind], 0, rows, 0)
            for cutoff in (TINY, 0.5):
                mst = None
                for rep in range(a.reps):
                    _, st = t.mst(cutoff)
                    emit(call="mst", table=what, cutoff=cutoff, rep=rep, rounds=int(st["rounds"]), scans=scans_of(st, rows), edges=int(st["edges"]),
                         kernel_ms=st["kernel_ms"], round_ms=st["round_ms"], sort_ms=st["sort_ms"], wall_ms=st["wall_ms"], clock_mhz=st["clock_mhz"])
                    if mst is None or st["scan_kernel_ms"][0] < mst["scan_kernel_ms"][0]:
                        mst = st
                for mp in min_pts:
                    knn = forest = None
                    for rep in range(a.reps):
                        st = {}
                        t.knn(mp - 1, cutoff, stats=st)
                        emit(call="knn", table=what, k=mp - 1, cutoff=cutoff, rep=rep, kernel_ms=st["kernel_ms"], wall_ms=st["wall_ms"],
                             launches=int(st["launches"]), inserts=int(st["inserts"]), clock_mhz=st["clock_mhz"],
                             fraction_of_ceiling=rows * rows / (st["kernel_ms"] * 1e-3) / ceiling(st["clock_mhz"]) if st["clock_mhz"] else None)
                        if knn is None or st["kernel_ms"] < knn["kernel_ms"]:
                            knn = st
                        edges, core, st = t.mreach_mst(mp, cutoff)
                        emit(call="mreach_mst", table=what, min_pts=mp, cutoff=cutoff, rep=rep, rounds=int(st["rounds"]), scans=scans_of(st, rows),
                             edges=int(st["edges"]), tied_edges=int(len(edges) - len(np.unique(edges["score"]))) if len(edges) else 0,
                             core_rows=int(st["core_rows"]), core_launches=int(st["core_launches"]), core_inserts=int(st["core_inserts"]),
                             core_kernel_ms=st["core_kernel_ms"], core_tail_ms=st["core_tail_ms"], kernel_ms=st["kernel_ms"], round_ms=st["round_ms"],
                             sort_ms=st["sort_ms"], wall_ms=st["wall_ms"], clock_mhz=st["clock_mhz"])
                        if forest is None or st["scan_kernel_ms"][0] < forest["scan_kernel_ms"][0]:
                            forest = st
                    t0 = time.perf_counter()
                    out = capi.mst_hdbscan(edges, rows, cutoff, mp)
                    select_ms = (time.perf_counter() - t0) * 1e3
                    emit(summary=what, min_pts=mp, cutoff=cutoff, scan1_kernel_ms=forest["scan_kernel_ms"][0], mst_scan1_kernel_ms=mst["scan_kernel_ms"][0],
                         scan1_over_mst_scan1=forest["scan_kernel_ms"][0] / mst["scan_kernel_ms"][0], scans_kernel_ms=forest["kernel_ms"],
                         mst_scans_kernel_ms=mst["kernel_ms"], core_kernel_ms=forest["core_kernel_ms"], knn_kernel_ms=knn["kernel_ms"],
                         core_over_knn=forest["core_kernel_ms"] / knn["kernel_ms"], core_tail_ms=forest["core_tail_ms"],
                         forest_wall_ms=forest["wall_ms"], mst_wall_ms=mst["wall_ms"], select_host_ms=select_ms, clusters=int(len(out[2])),
                         noise=int((out[0] == capi.HDBSCAN_NOISE).sum()))
            t.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
