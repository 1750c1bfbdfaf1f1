"""Time gsim_db_label_sums (HIP events inside the library: the sort, the gather, all fold launches, D2H) on synthetic Morgan-shaped
tables, full and own-only, beside gsim_db_histogram's owner-tile kernel on the same table in the same run, and report pairs/s against
the VALU engine's ceiling (DESIGN.md sections 9, 16 and 29).

    python scripts/time_label_sums.py [--rows 100000,1000000] [--bits 1024] [--centres 1000] [--kmeans-iter 3] [--reps 2]
                                      [--out profiles/label_sums_time.txt]

Per table: labels from gsim_db_kmeans at --centres centres (--kmeans-iter assignments from evenly spaced rows), then (1) the full
pass, (2) the own-only pass (the medoid route), (3) gsim_db_histogram of the table against itself on the owner-tile route
(GSIM_HIST_STREAM_MAX_ROWS=0) with ten uniform edges -- its band sends a pair below edges[0] to bin 0 without the divide -- and with a
first edge of 2^-20, under which only a pair without a common bit is spared the divide: the kernel closest to one that divides for every
pair.  No threshold is set.  The summary line gives the full pass's rate over either histogram's and its silhouette and medoids' host ms.
Ceiling: as scripts/time_components.py -- 8.8 cycles per wave64 v_and + v_bcnt pair per SIMD, 1024 SIMDs, 64 pairs per instruction
pair, rows padded to WP words -- at the clock the kernels themselves measured (clock_mhz)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--kmeans-iter", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_sums_time.txt"))
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

    def rate_of(pairs, ms, mhz):
        r = pairs / (ms * 1e-3) if ms else None
        return r, (r / ceiling(mhz) if r and mhz else None)

    os.environ["GSIM_HIST_STREAM_MAX_ROWS"] = "0"  # (read once per handle, when it is created: the histograms below take the owner-tile route)
    for n in [int(x) for x in a.rows.split(",")]:
        what = "morgan %d x %d" % (n, a.bits)
        t = capi.Table(a.bits).generate(0xC0FFEE, capi.SYNTH_MORGAN, 0, n, 0)
        m = min(a.centres, n)
        init = np.stack([t.row(i * (n // m)) for i in range(m)])
        _, labels, _, sizes, ks = t.kmeans(init, a.kmeans_iter)
        emit(call="kmeans", table=what, centres=m, iterations=int(ks["iterations"]), wall_ms=ks["wall_ms"], nonempty=int((sizes > 0).sum()),
             largest=int(sizes.max()), in_cluster_pairs=int((sizes.astype(np.int64) ** 2).sum()) - n)
        t.label_sums(labels[:4096], m, 0, min(n, 4096))  # warm-up: loads the kernels
        t.label_sums(labels[:4096], m, 0, min(n, 4096), own_only=True)
        best = {}
        for own_only in (False, True):
            for rep in range(a.reps):
                own, other, other_q, z, st = t.label_sums(labels, m, own_only=own_only)
                r, f = rate_of(st["pairs"], st["kernel_ms"], st["clock_mhz"])
                emit(call="label_sums", table=what, own_only=int(own_only), rep=rep, pairs=int(st["pairs"]), launches=int(st["launches"]),
                     sort_ms=st["sort_ms"], gather_ms=st["gather_ms"], kernel_ms=st["kernel_ms"], d2h_ms=st["d2h_ms"], wall_ms=st["wall_ms"],
                     clock_mhz=st["clock_mhz"], pairs_per_s=r, fraction_of_ceiling=f)
                if own_only not in best or st["kernel_ms"] < best[own_only][0]:
                    best[own_only] = (st["kernel_ms"], r, f)
            if not own_only:
                t0 = time.perf_counter()
                sil, lmean, mean = capi.label_silhouette(labels, own, other, other_q, z)
                sil_ms = (time.perf_counter() - t0) * 1e3
            else:
                t0 = time.perf_counter()
                med = capi.label_medoids(labels, own, m)
                med_ms = (time.perf_counter() - t0) * 1e3
        emit(call="host", table=what, silhouette_ms=sil_ms, mean_silhouette=mean, medoids_ms=med_ms, medoids=int((med != capi.LABEL_NONE).sum()))
        hist = {}
        for name, edges in (("ten uniform edges", np.arange(1, 11, dtype=np.float32) / np.float32(10)),
                            ("first edge 2^-20", np.concatenate([[np.float32(2.0 ** -20)], np.arange(1, 10, dtype=np.float32) / np.float32(10)]))):
            edges = edges.astype(np.float32)
            t.histogram(t, edges, row_end=min(n, 1024), per_row=False, exclude_self=True)  # warm-up
            for rep in range(a.reps):
                st = {}
                _, total = t.histogram(t, edges, per_row=False, exclude_self=True, stats=st)
                r, f = rate_of(st["pairs"], st["tile_ms"], st["clock_mhz"])
                emit(call="histogram_tiles", table=what, edges=name, rep=rep, pairs=int(st["pairs"]), launches=int(st["tile_launches"]),
                     tile_ms=st["tile_ms"], wall_ms=st["wall_ms"], clock_mhz=st["clock_mhz"], pairs_per_s=r, fraction_of_ceiling=f,
                     bin0_share=float(total[0]) / float(total.sum()))
                if name not in hist or st["tile_ms"] < hist[name][0]:
                    hist[name] = (st["tile_ms"], r, f)
        emit(summary=what, full_kernel_ms=best[False][0], full_pairs_per_s=best[False][1], full_fraction_of_ceiling=best[False][2],
             own_only_kernel_ms=best[True][0], own_only_pairs_per_s=best[True][1], own_only_fraction_of_ceiling=best[True][2],
             **{"hist_%s_ms" % k.replace(" ", "_"): v[0] for k, v in hist.items()},
             **{"hist_%s_fraction_of_ceiling" % k.replace(" ", "_"): v[2] for k, v in hist.items()},
             **{"full_rate_over_hist_%s" % k.replace(" ", "_"): best[False][1] / v[1] for k, v in hist.items()})
        t.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
