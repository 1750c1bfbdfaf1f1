"""Time gsim_db_histogram / gsim_db_histogram_queries (HIP events inside the library) on synthetic tables made on the device, beside
the unchanged kernels that are its yardsticks on the same table in the same run.

    python scripts/time_histogram.py --step tile      [--rows 1000000] [--bits 1024] [--kinds sparse,morgan] [--edges 10,64,128] [--owners 0]
    python scripts/time_histogram.py --step stream    [--rows 100000000] [--kinds sparse,morgan]
    python scripts/time_histogram.py --step crossover [--rows 1000000] [--kinds morgan] [--lefts 1,2,4,8,16,32,64,128]

tile:      the owner-tile route (GSIM_HIST_STREAM_MAX_ROWS=0) on a self histogram of the owner rows [0, OWNERS) (0: the whole table)
           with B uniform edges k / B: tile ms, launches, pairs/s and the fraction of the VALU ceiling at the clock the kernel itself
           measured, beside the pair rates of gsim_db_knn's fold kernel (k = 8, cutoff 0.5) over the same owner rows and of the
           neighbours tile kernel (a rectangle of --nbr-rows rows at cutoff 0.7).
stream:    the streaming route with 1 and 8 left rows, ms per pass, beside gsim_db_join_queries at cutoff 1.0 (the same loop with a
           filter that keeps nothing on i.i.d. rows: the floor) and gsim_db_search of one query (host clock); the peeled LDS add and
           the naive one (GSIM_HIST_NAIVE_ADD=1) side by side.
crossover: both routes for a growing number of left rows; the first count at which the tile route is the faster one.
Ceiling: 8.8 cycles per wave64 word-pair instruction pair per SIMD, 1024 SIMDs, 64 pairs per instruction pair, rows padded to WP
words (scripts/time_neighbors.py).  Knobs are read once per handle: every variant is a table of its own, generated from the same
seed."""
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
SEED = 0xC0FFEE
OUT = []


def emit(**rec):
    print(json.dumps(rec), flush=True)
    OUT.append(rec)


def generate(bits, kind, n, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return capi.Table(bits).generate(SEED, KINDS[kind], 0, n, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def grid(b):
    return (np.arange(1, b + 1, dtype=np.float32) / np.float32(b)).astype(np.float32)


def step_tile(a):
    wp = 4
    while wp < a.bits // 32:
        wp *= 2
    n = a.rows
    owners = a.owners if a.owners > 0 else n
    for kind in a.kinds.split(","):
        t = generate(a.bits, kind, n, GSIM_HIST_STREAM_MAX_ROWS=0)
        nb = min(a.nbr_rows, owners)
        t.neighbors(0.7, row_begin=0, row_end=min(nb, 4096))  # warm-up: sizes the pair buffer, loads the kernels
        st = {}
        t.neighbors(0.7, row_begin=0, row_end=nb, stats=st)
        nbr_rate = nb * n / (st["tile_ms"] * 1e-3)
        emit(what="neighbors_rectangle", kind=kind, rows=n, bits=a.bits, left_rows=nb, cutoff=0.7, tile_ms=st["tile_ms"],
             launches=int(st["launches"]), launches_rerun=int(st["launches_rerun"]), clock_mhz=st["clock_mhz"], pairs_per_s=nbr_rate,
             fraction_of_ceiling=nbr_rate / (1024 * st["clock_mhz"] * 1e6 / 8.8 * 64 / wp))
        t.knn(8, 0.5, row_begin=0, row_end=min(owners, 1024))
        st = {}
        t.knn(8, 0.5, row_begin=0, row_end=owners, stats=st)
        knn_rate = st["pairs"] / (st["kernel_ms"] * 1e-3)
        emit(what="knn_fold", kind=kind, rows=n, bits=a.bits, owners=owners, k=8, cutoff=0.5, kernel_ms=st["kernel_ms"],
             launches=int(st["launches"]), clock_mhz=st["clock_mhz"], pairs_per_s=knn_rate,
             fraction_of_ceiling=knn_rate / (1024 * st["clock_mhz"] * 1e6 / 8.8 * 64 / wp))
        for b in [int(x) for x in a.edges.split(",")]:
            edges = grid(b)
            t.histogram(t, edges, row_end=min(owners, 1024), per_row=False)  # warm-up
            st = {}
            _, total = t.histogram(t, edges, row_end=owners, per_row=False, stats=st)
            rate = st["pairs"] / (st["tile_ms"] * 1e-3)
            emit(what="histogram_tiles", kind=kind, rows=n, bits=a.bits, owners=owners, edges=b, tile_ms=st["tile_ms"],
                 launches=int(st["tile_launches"]), mean_launch_ms=st["tile_ms"] / max(st["tile_launches"], 1), reduce_ms=st["reduce_ms"],
                 d2h_ms=st["d2h_ms"], call_ms=st["wall_ms"], clock_mhz=st["clock_mhz"], pairs_per_s=rate,
                 fraction_of_ceiling=rate / (1024 * st["clock_mhz"] * 1e6 / 8.8 * 64 / wp), rate_over_knn_fold=rate / knn_rate,
                 rate_over_neighbors=rate / nbr_rate, bin0_share=float(total[0]) / float(total.sum()))
        t.close()


def stream_ms(t, q, edges, reps=3):
    t.histogram(q, edges, per_row=False)
    best = None
    for _ in range(reps):
        st = {}
        t.histogram(q, edges, per_row=False, stats=st)
        assert st["rows_streamed"] == len(q), st
        best = st["stream_ms"] if best is None else min(best, st["stream_ms"])
    return best / len(q), int(st["stream_launches"]) // len(q)


def step_stream(a):
    n = a.rows
    edges = grid(10)
    for kind in a.kinds.split(","):
        q = np.stack([capi.synth_row(SEED, KINDS[kind], r, a.bits) for r in range(8)])
        t = generate(a.bits, kind, n, GSIM_HIST_STREAM_MAX_ROWS=1 << 30, GSIM_JOIN_STREAM_MAX_ROWS=1 << 30)
        for nl in (1, 8):
            ms, launches = stream_ms(t, q[:nl], edges)
            t.join(q[:nl], 1.0)
            st = {}
            t.join(q[:nl], 1.0, stats=st)
            t.search(q[:1], 10, 0.0)
            w0 = time.perf_counter()
            for _ in range(5):
                t.search(q[:1], 10, 0.0)
            search_ms = (time.perf_counter() - w0) * 1e3 / 5
            emit(what="histogram_stream", kind=kind, rows=n, bits=a.bits, left_rows=nl, edges=10, add="peeled", ms_per_pass=ms,
                 launches_per_pass=launches, gb_per_s=n * a.bits / 8 / ms * 1e-6, join_ms_per_pass=st["stream_ms"] / nl,
                 join_pairs=int(st["pairs"]), over_join=ms / (st["stream_ms"] / nl), search_ms=search_ms)
        t.close()
        t = generate(a.bits, kind, n, GSIM_HIST_STREAM_MAX_ROWS=1 << 30, GSIM_HIST_NAIVE_ADD=1)
        for nl in (1, 8):
            ms, launches = stream_ms(t, q[:nl], edges)
            emit(what="histogram_stream", kind=kind, rows=n, bits=a.bits, left_rows=nl, edges=10, add="naive", ms_per_pass=ms,
                 launches_per_pass=launches, gb_per_s=n * a.bits / 8 / ms * 1e-6)
        t.close()


def step_crossover(a):
    n = a.rows
    edges = grid(10)
    lefts = [int(x) for x in a.lefts.split(",")]
    for kind in a.kinds.split(","):
        q = np.stack([capi.synth_row(SEED, KINDS[kind], r, a.bits) for r in range(max(lefts))])
        ts = generate(a.bits, kind, n, GSIM_HIST_STREAM_MAX_ROWS=1 << 30)
        tt = generate(a.bits, kind, n, GSIM_HIST_STREAM_MAX_ROWS=0)
        first = None
        for nl in lefts:
            res = {}
            for name, t in (("stream", ts), ("tiles", tt)):
                t.histogram(q[:nl], edges, per_row=False)
                best = None
                for _ in range(3):
                    st = {}
                    t.histogram(q[:nl], edges, per_row=False, stats=st)
                    best = st["wall_ms"] if best is None else min(best, st["wall_ms"])
                res[name] = dict(call_ms=best, kernel_ms=st["stream_ms"] + st["tile_ms"], launches=int(st["stream_launches"] + st["tile_launches"]))
            if first is None and res["tiles"]["call_ms"] < res["stream"]["call_ms"]:
                first = nl
            emit(what="histogram_crossover", kind=kind, rows=n, bits=a.bits, left_rows=nl, stream=res["stream"], tiles=res["tiles"])
        emit(what="histogram_crossover_summary", kind=kind, rows=n, bits=a.bits, tiles_first_faster_at=first)
        ts.close()
        tt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("tile", "stream", "crossover"), required=True)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--kinds", default=None)
    ap.add_argument("--edges", default="10,64,128")
    ap.add_argument("--owners", type=int, default=0, help="tile: only the owner rows [0, OWNERS) (0: the whole table)")
    ap.add_argument("--nbr-rows", type=int, default=131072, help="tile: rows of the neighbours yardstick's rectangle")
    ap.add_argument("--lefts", default="1,2,4,8,16,32,64,128")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rows is None:
        a.rows = 100_000_000 if a.step == "stream" else 1_000_000
    if a.kinds is None:
        a.kinds = "morgan" if a.step == "crossover" else "sparse,morgan"
    {"tile": step_tile, "stream": step_stream, "crossover": step_crossover}[a.step](a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(OUT, f, indent=1)


if __name__ == "__main__":
    main()
