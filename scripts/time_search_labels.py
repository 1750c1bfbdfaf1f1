"""Time gsim_db_search_labels (HIP events inside the library: all scan launches; the finish, the ranking and the emission; D2H) on
synthetic Morgan-shaped tables, beside gsim_db_search on the same table in the same run and the two compositions the call replaces
(DESIGN.md section 30).

    python scripts/time_search_labels.py [--rows 1000000,100000000] [--bits 1024] [--reps 3] [--out profiles/search_labels_time.txt]

Per table and per configuration -- nlabels 1000 and 10 000 (route LDS) and N / 10 (route global); labels in random order and in
cluster order (label = row * nlabels // N); cutoff 0 and a selective cutoff with the per-label counts asked for; nq = 1 and nq = 16
-- one warm-up call, then --reps calls: the median and the least scan time per query and what fraction of 8 TB/s that is over
(row bytes + 4) x N bytes per table pass (the bytes the algorithm needs: the rows and their labels, once per pass, whatever the
number of queries that share it).  The selective cutoff is the score of the query's hit number min(N / 100, 100 000).
Yardsticks, never from the code under test: gsim_db_search at k = 1000 (nq = 1 through the single-query path, nq = 16 as one
multi-query call); one gsim_db_search_rows(k = 1) per label for 100 labels of the random 1000-label vector, times nlabels / 100;
gsim_db_search at k = 100 000 and grouping its hits by label on the host, with the number of labels that list misses."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

PEAK = 8e12  # bytes/s, the figure DESIGN.md quotes every scan against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,100000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_labels_time.txt"))
    a = ap.parse_args()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    row_bytes = a.bits // 8
    for n in [int(x) for x in a.rows.split(",")]:
        what = "morgan %d x %d" % (n, a.bits)
        t = capi.Table(a.bits).generate(0xC0FFEE, capi.SYNTH_MORGAN, 0, n, 0)
        q = np.stack([t.row((i * 7919 + 13) % n) for i in range(16)])
        pass_bytes = (row_bytes + 4) * n

        def timed(fn):
            fn()
            out = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = fn()
                out.append((r, (time.perf_counter() - t0) * 1e3))
            return out

        # the yardstick: gsim_db_search, k = 1000
        for nq in (1, 16):
            walls = [w for _, w in timed(lambda: t.search(q[:nq], 1000))]
            rec = dict(table=what, call="gsim_db_search k=1000", nq=nq, wall_ms_per_query_median=float(np.median(walls)) / nq,
                       wall_ms_per_query_min=min(walls) / nq)
            if nq == 1:  # (how many table passes a multi-query call makes is the library's business: no bytes to divide by)
                rec["fraction_of_8TBs"] = row_bytes * n / PEAK / (min(walls) * 1e-3)
            emit(**rec)
        hits, _ = t.search(q[:1], min(max(n // 100, 1), 100000))
        selective = float(hits[0]["score"][-1])

        rng = np.random.default_rng(11)
        for nlabels in (1000, 10000, n // 10):
            for order in ("random", "cluster"):
                labels = (rng.integers(0, nlabels, n, dtype=np.int64) if order == "random" else np.arange(n, dtype=np.int64) * nlabels // n).astype(np.uint32)
                with t.labelset(labels, nlabels) as ls:
                    for cutoff, per_label in ((0.0, False), (selective, True)):
                        for nq in (1, 16):
                            runs = timed(lambda: t.search_labels(ls, q[:nq], 100, cutoff, per_label=per_label, stats=True))
                            st = [r["stats"] for r, _ in runs]
                            scan = [s["scan_ms"] for s in st]
                            passes = st[0]["passes"]
                            emit(table=what, call="gsim_db_search_labels", nlabels=nlabels, order=order, cutoff=cutoff, counting=per_label, nq=nq,
                                 route="lds" if st[0]["passes_lds"] else "global", passes=passes, launches=st[0]["launches"],
                                 scan_ms_per_query_median=float(np.median(scan)) / nq, scan_ms_per_query_min=min(scan) / nq,
                                 finish_ms_per_query=float(np.median([s["finish_ms"] for s in st])) / nq,
                                 d2h_ms_per_query=float(np.median([s["d2h_ms"] for s in st])) / nq,
                                 wall_ms_per_query_median=float(np.median([w for _, w in runs])) / nq,
                                 fraction_of_8TBs=passes * pass_bytes / PEAK / (min(scan) * 1e-3))
                    if nlabels == 1000 and order == "random":
                        # composition 1: one row-set search per label, 100 labels, extrapolated to all of them
                        some = np.flatnonzero(labels < 100).astype(np.uint32)
                        sets = [t.rowset(rows=some[labels[some] == l]) for l in range(100)]
                        t0 = time.perf_counter()
                        for rs in sets:
                            t.search_rows(rs, q[:1], 1)
                        per = (time.perf_counter() - t0) * 1e3 / 100
                        for rs in sets:
                            rs.close()
                        emit(table=what, call="gsim_db_search_rows k=1, one per label", nlabels=nlabels, labels_timed=100, wall_ms_per_label=per,
                             wall_ms_per_query_extrapolated=per * nlabels)
                    if order == "random":
                        # composition 2: a long hit list grouped on the host -- not exact: it misses the labels whose best lies below it
                        k = min(100000, n)
                        t0 = time.perf_counter()
                        hits, _ = t.search(q[:1], k)
                        found = len(np.unique(labels[hits[0]["row"]]))
                        wall = (time.perf_counter() - t0) * 1e3
                        nonempty = len(np.unique(labels))
                        emit(table=what, call="gsim_db_search k=100000 + host grouping", nlabels=nlabels, wall_ms_per_query=wall, labels_found=found,
                             labels_missed=nonempty - found)
                del labels
        t.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
