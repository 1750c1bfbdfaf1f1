"""Time gsim_rowhash_* on generated Morgan-shaped tables.

    python scripts/time_rowhash.py [--rows 1000000,100000000] [--bits 1024] [--reps 3] [--out FILE.json]

For every table size N, on one handle:
  search     one gsim_db_search (k = 1000) and gsim_popindex_create: what a pass over the table costs on this box
  build      gsim_rowhash_create: the HIP-event ms of its passes (insert + finish), the wall ms, the groups found, and the build's
             bytes/s (N x row bytes over the event ms) against 8 TB/s; best of --reps
  find       gsim_rowhash_find of 1, 1024 and 1 M queries (half of them rows of the table, half absent): wall ms, beside
             gsim_db_search_each at cutoff 1.0, k = 1 for the first 1 and 64 of them, per query
and once a build on 1 M identical rows: every row meets in one slot.  The split of the build between the inserting pass and the
finish is read from a kernel trace of this script (profiles/rowhash_time.txt), not from the library."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import oracle_lib as O  # noqa: E402  (the generator's host twin: the queries are rows of the table)
from gpusimilarity_amd import capi  # noqa: E402

SEED = 0x20000
PEAK = 8e12


def emit(rec, sink):
    print(json.dumps(rec), flush=True)
    sink.append(rec)


def best(fn, reps):
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ms = (time.perf_counter() - t0) * 1e3
        if out is None or ms < out[0]:
            out = (ms, r)
    return out


def build(t, reps):
    st = None
    for _ in range(reps):
        with t.rowhash() as ix:
            s = ix.stats()
        if st is None or s["kernel_ms"] < st["kernel_ms"]:
            st = s
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,100000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    W, sink = a.bits // 32, []
    for n in [int(x) for x in a.rows.split(",")]:
        t = capi.Table(a.bits).generate(SEED, capi.SYNTH_MORGAN, 0, n, 0)
        nq = min(1 << 20, n)
        present = O.synth_rows_mt(SEED, O.KIND_MORGAN, 0, nq, W, 16)
        queries = present.copy()
        queries[1::2, 0] ^= np.uint32(0x80000001)  # every other query: no longer a row of the table (but for a rare coincidence)
        bufs = t.make_search_buffers(1, 1000)
        t.search_into(queries[:1], 1000, bufs)
        ms, _ = best(lambda: t.search_into(queries[:1], 1000, bufs), a.reps + 2)
        emit(dict(what="gsim_db_search", rows=n, k=1000, ms=ms, bytes_per_s_over_peak=n * W * 4 / (ms * 1e-3) / PEAK), sink)
        ms, _ = best(lambda: t.popindex().close(), a.reps)
        emit(dict(what="gsim_popindex_create", rows=n, wall_ms=ms), sink)
        st = build(t, a.reps)
        emit(dict(what="gsim_rowhash_create", bytes_per_s_over_peak=n * W * 4 / (st["kernel_ms"] * 1e-3) / PEAK, **st), sink)
        with t.rowhash() as ix:
            for m in (1, 1024, nq):
                ix.find(queries[:m])
                ms, (row, _) = best(lambda: ix.find(queries[:m]), a.reps)
                emit(dict(what="gsim_rowhash_find", rows=n, queries=m, wall_ms=ms, us_per_query=ms * 1e3 / m, found=int((row != capi.ROW_NONE).sum())), sink)
            for m in (1, 64):
                b = t.make_search_buffers(m, 1)
                t.search_each_into(queries[:m], 1, b, 1.0)
                ms, _ = best(lambda: t.search_each_into(queries[:m], 1, b, 1.0), a.reps)
                emit(dict(what="gsim_db_search_each at cutoff 1.0", rows=n, queries=m, wall_ms=ms, us_per_query=ms * 1e3 / m), sink)
        t.close()
    n = 1 << 20
    same = capi.Table(a.bits).add_rows(np.tile(O.synth_rows(SEED, O.KIND_MORGAN, 0, 1, W), (n, 1))).finalize(0, 1)
    st = build(same, a.reps)
    emit(dict(what="gsim_rowhash_create, identical rows", **st), sink)
    same.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(sink, f, indent=1)


if __name__ == "__main__":
    main()
