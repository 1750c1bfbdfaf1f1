"""Time gsim_db_search_bounded on generated Morgan-shaped tables.

    python scripts/time_popindex.py [--rows 1000000,100000000] [--bits 1024] [--k 1000] [--queries 8] [--reps 3] [--out FILE.json]

For every table size N:
  build      wall ms of gsim_popindex_create without and with the popcount-ordered copy of the rows (their difference is the copy's
             phase: the gathered permutation of N rows); best of --reps
  search     gsim_db_search (the batch pass where it applies) and gsim_db_search_each (one query at a time: the parent's route for a
             caller that wants what the bounded call gives) on the same handle, ms per query
  bounded    for every cutoff of --cutoffs, with approx (the cutoff window, one scan) and -- at cutoff 0 and with a cutoff -- without
             it (top-k narrowing), for the index with the copy (streams), without it under the default gather rule, and without it with
             the gather forced (GSIM_SUBSET_GATHER_MAX_PERMILLE=1000): ms per query (wall and HIP events), the bound tables' ms, rows
             scanned over N, the stages and routes taken, and the window scan's bytes per second against 8 TB/s
  crossing   per route, the window fraction at which a linear fit of ms per query over the fraction scanned (one-stage queries of
             that route only) meets gsim_db_search_each's ms per query -- beyond it the plain search is the faster choice.  A fit needs
             two windows that the route answers in one stage: on these tables the default cutoffs give the streamed route one (0.9;
             the windows of 0.7 and below lie past its 3/4-of-N limit) and "crossing: null" -- pass more cutoffs between 0.75 and
             0.95 (--cutoffs 0,0.5,0.8,0.85,0.9,0.95) for the streamed route's crossing"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

SEED = 0x20000
KNOB = "GSIM_SUBSET_GATHER_MAX_PERMILLE"
PEAK = 8e12


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def emit(rec, sink):
    print(json.dumps(rec), flush=True)
    sink.append(rec)


def build_ms(t, rows, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        ix = t.popindex(rows=rows)
        ms = (time.perf_counter() - t0) * 1e3
        ix.close()
        best = ms if best is None else min(best, ms)
    return best


def search_ms(t, queries, k, cutoff, reps, each):
    bufs = t.make_search_buffers(len(queries), k)
    fn = t.search_each_into if each else t.search_into
    fn(queries, k, bufs, cutoff)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(queries, k, bufs, cutoff)
        ms = (time.perf_counter() - t0) * 1e3 / len(queries)
        best = ms if best is None else min(best, ms)
    return best


def bounded(t, ix, queries, k, cutoff, approx, reps):
    t.search_bounded(ix, queries[:1], k, cutoff, approx=approx)
    best = None
    for _ in range(reps):
        _, _, st = t.search_bounded(ix, queries, k, cutoff, approx=approx, stats=True)
        if best is None or st["wall_ms"] < best["wall_ms"]:
            best = st
    return best


def run(n, a, sink):
    bits, k, nq = a.bits, a.k, a.queries
    row_bytes = bits // 8
    queries = np.stack([capi.synth_row(SEED, capi.SYNTH_MORGAN, n + i, bits) for i in range(nq)])
    tables = {}
    for name, permille in (("default", None), ("gather forced", "1000")):
        with env(**{KNOB: permille}):
            tables[name] = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, n, 0)
    t = tables["default"]
    plain_ms, copy_ms = build_ms(t, False, a.reps), build_ms(t, True, a.reps)
    emit(dict(section="build", rows=n, bits=bits, order_ms=plain_ms, with_copy_ms=copy_ms, copy_phase_ms=copy_ms - plain_ms), sink)
    indexes = {"copy": (t, t.popindex(rows=True)), "no copy": (t, t.popindex()), "no copy, gather forced": (tables["gather forced"], tables["gather forced"].popindex())}
    points = {name: [] for name in indexes}
    each_at = {}
    for cutoff in a.cutoffs:
        each_at[cutoff] = search_ms(t, queries, k, cutoff, a.reps, True)
        emit(dict(section="search", rows=n, bits=bits, k=k, cutoff=cutoff, search_ms=search_ms(t, queries, k, cutoff, a.reps, False),
                  search_each_ms=each_at[cutoff]), sink)
        for name, (tab, ix) in indexes.items():
            for approx in (True, False):
                st = bounded(tab, ix, queries, k, cutoff, approx, a.reps)
                frac = st["rows_scanned"] / (n * nq)
                scans = st["queries_one_stage"] + 2 * st["queries_two_stage"] + st["queries_plain"]
                rec = dict(section="bounded", rows=n, bits=bits, k=k, cutoff=cutoff, index=name, approx=approx, ms=st["wall_ms"] / nq,
                           kernel_ms=st["kernel_ms"] / nq, bounds_ms=st["bounds_ms"] / nq, rows_scanned_over_n=frac,
                           window_over_n=st["rows_window"] / (n * nq), one_stage=st["queries_one_stage"], two_stage=st["queries_two_stage"],
                           plain=st["queries_plain"], over_search_each=st["wall_ms"] / nq / each_at[cutoff],
                           scan_bytes_per_s=st["rows_scanned"] * (row_bytes + 4) / (st["kernel_ms"] * 1e-3) if st["kernel_ms"] > 0 else None)
                if rec["scan_bytes_per_s"]:
                    rec["of_8_tb_s"] = rec["scan_bytes_per_s"] / PEAK
                emit(rec, sink)
                if approx and st["queries_plain"] == 0 and st["queries_two_stage"] == 0 and scans:
                    points[name].append((frac, st["wall_ms"] / nq, each_at[cutoff]))
    for name, pts in points.items():
        pts = [p for p in pts if p[0] > 0]
        if len(pts) < 2:
            emit(dict(section="crossing", rows=n, index=name, crossing=None, why="fewer than two one-stage points"), sink)
            continue
        f, ms, each = (np.array(x) for x in zip(*pts))
        slope, icpt = np.polyfit(f, ms, 1)
        target = float(np.median(each))
        cross = (target - icpt) / slope if slope > 0 else None
        emit(dict(section="crossing", rows=n, index=name, points=[[float(x), float(y)] for x, y in zip(f, ms)], ms_per_fraction=float(slope),
                  ms_at_zero=float(icpt), search_each_ms=target, crossing=cross, with_margin=None if cross is None else cross / 1.1), sink)
    for tab, ix in indexes.values():
        ix.close()
    for tab in tables.values():
        tab.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,100000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cutoffs", default="0,0.3,0.5,0.7,0.9")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.cutoffs = [float(x) for x in a.cutoffs.split(",")]
    sink = []
    for n in (int(x) for x in a.rows.split(",")):
        run(n, a, sink)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(sink, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
