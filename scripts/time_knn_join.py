"""Time gsim_db_knn_join (HIP events inside the library: the fold launches, the merge, the CSR build, D2H) on synthetic tables made on
the device, beside its yardsticks on the same tables in the same run, and report pairs/s against the VALU engine's ceiling
 at the clock the fold kernel itself measured.

    python scripts/time_knn_join.py [--rows 1000000] [--bits 1024] [--kinds morgan,sparse] [--ks 8,32,128] [--lefts 512,4096]
                                    [--steps a,b,c] [--reps 3] [--segments 0]

  a  few left rows against a long table: per kind, left size, k and cutoff (the smallest positive float, and 0.5) the split call
     under the automatic plan -- S, fold + merge ms (the best of --reps calls, and every call's), inserts, pairs/s, the fraction of
     the ceiling -- beside (1) gsim_db_search with the same left rows as queries, 256 per call, at k: the route to these lists
     without the join; and, at 512 left rows, (2) gsim_db_knn at k on a 512-row range of the table: the unsplit fold on the same
     amount of work (its lists differ: the table's own rows).
  b  --rows left rows (a second generated table, another seed) against the table, one segment, beside gsim_db_knn on the table: the
     same scheme, so the pair rates should match.  k = 8.
  c  the merge alone: its ms and its share of fold + merge at GSIM_KNN_JOIN_SEGMENTS = 5 and under the automatic plan, for case
     a's shapes at k = 8 and 128.
--segments S > 0 runs step a with GSIM_KNN_JOIN_SEGMENTS = S instead of the automatic plan (what more, or fewer, segments cost).
Ceiling: 8.8 cycles per wave64 word-pair instruction pair per SIMD, 1024 SIMDs, 64 pairs per instruction pair, rows padded to WP
words (scripts/time_neighbors.py).  The stats carry no per-launch times: the longest launch comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/time_knn_join.py ...)."""
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
SEED, LEFT_SEED = 0xC0FFEE, 0xDECAF


def emit(**rec):
    print(json.dumps(rec), flush=True)
    return rec


def generate(bits, seed, kind, rows, segments=None):
    """(the knobs are read once per handle, when it is created)"""
    old = os.environ.pop("GSIM_KNN_JOIN_SEGMENTS", None)
    if segments is not None:
        os.environ["GSIM_KNN_JOIN_SEGMENTS"] = str(segments)
    try:
        return capi.Table(bits).generate(seed, kind, 0, rows, 0)
    finally:
        os.environ.pop("GSIM_KNN_JOIN_SEGMENTS", None)
        if old is not None:
            os.environ["GSIM_KNN_JOIN_SEGMENTS"] = old


def join_calls(t, lt, nl, k, cutoff, reps):
    """-> the stats of `reps` calls after one warm-up, the one with the least fold + merge time first"""
    t.knn_join(lt, k, cutoff, row_end=min(nl, 256))
    runs = []
    for _ in range(reps):
        st = {}
        t.knn_join(lt, k, cutoff, row_end=nl, stats=st)
        runs.append(st)
    return sorted(runs, key=lambda s: s["kernel_ms"] + s["merge_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--kinds", default="morgan,sparse")
    ap.add_argument("--ks", default="8,32,128")
    ap.add_argument("--lefts", default="512,4096")
    ap.add_argument("--steps", default="a,b,c")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--segments", type=int, default=0, help="step a: force this many column segments (0: the automatic plan)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W = a.bits // 32
    wp = 4
    while wp < W:
        wp *= 2
    n = a.rows
    ks = [int(x) for x in a.ks.split(",")]
    lefts = [int(x) for x in a.lefts.split(",")]
    steps = a.steps.split(",")
    out = []

    def ceiling(mhz):
        return 1024 * mhz * 1e6 / 8.8 * 64 / wp

    for kind in a.kinds.split(","):
        t = generate(a.bits, SEED, KINDS[kind], n, segments=a.segments if a.segments > 0 else None)
        lt = generate(a.bits, LEFT_SEED, KINDS[kind], max(lefts))
        if "a" in steps:
            q = np.stack([capi.synth_row(LEFT_SEED, KINDS[kind], r, a.bits) for r in range(max(lefts))])
            for nl in lefts:
                for k in ks:
                    for cutoff in (TINY, 0.5):
                        runs = join_calls(t, lt, nl, k, cutoff, a.reps)
                        st = runs[0]
                        ms = st["kernel_ms"] + st["merge_ms"]
                        rate = st["pairs"] / (ms * 1e-3)
                        # (1) the same rows as queries of gsim_db_search, 256 per call
                        t.search(q[:256], k, cutoff)
                        w0 = time.perf_counter()
                        for lo in range(0, nl, 256):
                            t.search(q[lo:min(lo + 256, nl)], k, cutoff)
                        search_ms = (time.perf_counter() - w0) * 1e3
                        rec = dict(what="knn_join", kind=kind, rows=n, bits=a.bits, left_rows=nl, k=k, cutoff=cutoff, segments=int(st["segments"]),
                                   fold_launches=int(st["fold_launches"]), fold_ms=st["kernel_ms"], merge_ms=st["merge_ms"], fold_merge_ms=ms,
                                   fold_merge_ms_all=[s["kernel_ms"] + s["merge_ms"] for s in runs], csr_ms=st["csr_ms"], d2h_ms=st["d2h_ms"],
                                   call_ms=st["wall_ms"], inserts=int(st["inserts"]), partial_entries=int(st["partial_entries"]),
                                   entries=int(st["entries"]), clock_mhz=st["clock_mhz"], pairs_per_s=rate,
                                   fraction_of_ceiling=rate / ceiling(st["clock_mhz"]), search_route_ms=search_ms,
                                   search_over_join_call=search_ms / st["wall_ms"])
                        if nl <= 512:
                            # (2) the unsplit fold on as many owner rows of the table itself
                            t.knn(k, cutoff, row_begin=0, row_end=64)
                            ks_ = {}
                            t.knn(k, cutoff, row_begin=0, row_end=nl, stats=ks_)
                            rec.update(knn_range_kernel_ms=ks_["kernel_ms"], knn_range_launches=int(ks_["launches"]),
                                       knn_range_call_ms=ks_["wall_ms"], knn_range_over_join_call=ks_["wall_ms"] / st["wall_ms"])
                        out.append(emit(**rec))
        if "c" in steps:
            t5 = generate(a.bits, SEED, KINDS[kind], n, segments=5)
            for nl in lefts:
                for k in (ks[0], ks[-1]):
                    for name, tab in (("5", t5), ("auto" if a.segments <= 0 else str(a.segments), t)):
                        st = join_calls(tab, lt, nl, k, TINY, a.reps)[0]
                        out.append(emit(what="merge", kind=kind, rows=n, bits=a.bits, left_rows=nl, k=k, cutoff=TINY, plan=name,
                                        segments=int(st["segments"]), fold_launches=int(st["fold_launches"]), fold_ms=st["kernel_ms"],
                                        merge_ms=st["merge_ms"], merge_share=st["merge_ms"] / (st["kernel_ms"] + st["merge_ms"]),
                                        partial_entries=int(st["partial_entries"]), entries=int(st["entries"])))
            t5.close()
        lt.close()
        if "b" in steps:
            big = generate(a.bits, LEFT_SEED, KINDS[kind], n)
            for cutoff in (TINY, 0.5):
                t.knn_join(big, 8, cutoff, row_end=1024)
                st = {}
                t.knn_join(big, 8, cutoff, stats=st)
                t.knn(8, cutoff, row_begin=0, row_end=1024)
                ks_ = {}
                t.knn(8, cutoff, stats=ks_)
                rate, knn_rate = st["pairs"] / (st["kernel_ms"] * 1e-3), ks_["pairs"] / (ks_["kernel_ms"] * 1e-3)
                out.append(emit(what="knn_join_full", kind=kind, rows=n, bits=a.bits, left_rows=n, k=8, cutoff=cutoff,
                                segments=int(st["segments"]), fold_launches=int(st["fold_launches"]), fold_ms=st["kernel_ms"],
                                merge_ms=st["merge_ms"], inserts=int(st["inserts"]), clock_mhz=st["clock_mhz"], pairs_per_s=rate,
                                fraction_of_ceiling=rate / ceiling(st["clock_mhz"]), knn_kernel_ms=ks_["kernel_ms"],
                                knn_launches=int(ks_["launches"]), knn_inserts=int(ks_["inserts"]), knn_clock_mhz=ks_["clock_mhz"],
                                knn_pairs_per_s=knn_rate, knn_fraction_of_ceiling=knn_rate / ceiling(ks_["clock_mhz"]),
                                rate_over_knn=rate / knn_rate))
            big.close()
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
