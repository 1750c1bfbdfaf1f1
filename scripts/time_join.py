"""Time gsim_db_join_queries / gsim_db_join route by route (HIP events inside the library) on synthetic Morgan-shaped tables
(DESIGN.md section 11).  Left rows are rows of the table's own series beyond its end (gsim_synth_row), so they have hits.

    python scripts/time_join.py [--sections stream,dense,tile,crossover] [--rows 100000000] [--small-rows 1000000]

  stream     one left row per call and 8 per call at cutoff 0.7 on --rows x 1024 bits: kernel time per pass, against
             gsim_db_search (k = 1000, same handle, same run: gsim_timing.scan_ms_sum / queries)
  dense      one left row per call at cutoff 0.15 (and 0.1): kept fraction and time per pass against the 0.7 pass of the same run
  tile       65 536 left rows (a second handle) x --small-rows: pairs/s of the tile launches against the VALU ceiling at the clock
             the kernel sampled (1024 SIMDs x f / 8.8 cycles x 64 pairs / words per row), whole call over tile time
  crossover  nl = 1 ... 256 through each route forced (GSIM_JOIN_STREAM_MAX_ROWS), on --small-rows and --rows at 1024 bits and on
             tables of the same bytes at 128 and 2048 bits; says which route the default knob takes and what it costs against
             the faster one"""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

SEED = 0x20000
STREAM, TILE = "2147483647", "0"


@contextlib.contextmanager
def knob(value):
    old = os.environ.pop("GSIM_JOIN_STREAM_MAX_ROWS", None)
    if value is not None:
        os.environ["GSIM_JOIN_STREAM_MAX_ROWS"] = value
    try:
        yield
    finally:
        os.environ.pop("GSIM_JOIN_STREAM_MAX_ROWS", None)
        if old is not None:
            os.environ["GSIM_JOIN_STREAM_MAX_ROWS"] = old


def make(n, bits, route):
    with knob(route):
        return capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, n, 0)


def left_rows(n, bits, count, first=0):
    return np.stack([capi.synth_row(SEED, capi.SYNTH_MORGAN, n + first + i, bits) for i in range(count)])


def emit(rec):
    print(json.dumps(rec), flush=True)


def per_pass(t, left, cutoff, per_call):
    """-> (kernel ms per pass of every call, pairs of every call, launches run again)"""
    ms, pairs, rerun = [], [], 0
    for i in range(0, len(left), per_call):
        st = {}
        t.join(left[i:i + per_call], cutoff, stats=st)
        ms.append((st["stream_ms"] + st["tile_ms"]) / per_call)
        pairs.append(int(st["pairs"]))
        rerun += int(st["launches_rerun"])
    return ms, pairs, rerun


def section_stream(a):
    n, bits = a.rows, 1024
    t = make(n, bits, STREAM)
    left = left_rows(n, bits, 16)
    t.join(left[:1], 0.7)  # warm-up: loads the kernels
    t.enable_timing(True)
    t.search(left[:1], 1000, 0.7)
    t.enable_timing(True)
    for q in left:
        t.search(q, 1000, 0.7)
    tm = t.timing()
    scan = tm["scan_ms_sum"] / tm["queries"]
    t.enable_timing(False)
    for per_call in (1, 8):
        ms, pairs, _ = per_pass(t, left, 0.7, per_call)
        emit(dict(section="stream", rows=n, bits=bits, cutoff=0.7, left_per_call=per_call, pass_ms_median=float(np.median(ms)),
                  pass_ms_min=min(ms), pass_ms_max=max(ms), search_scan_ms=scan, pass_over_search=float(np.median(ms)) / scan,
                  bar=1.10, fraction_of_8TBps=n * bits / 8 / (float(np.median(ms)) * 1e-3) / 8e12, pairs=sum(pairs)))
    if "dense" in a.sections:
        sparse = float(np.median(per_pass(t, left, 0.7, 1)[0]))
        for cutoff, count, bar in ((0.15, 16, 1.5), (0.1, 4, None)):
            t.join(left[:1], cutoff)  # sizes the pair buffer for this density
            for i in range(count):
                t.join(left[i:i + 1], cutoff)
            ms, pairs, rerun = per_pass(t, left[:count], cutoff, 1)
            emit(dict(section="dense", rows=n, bits=bits, cutoff=cutoff, kept_fraction=[p / n for p in pairs], pass_ms=ms,
                      pass_ms_median=float(np.median(ms)), pass_ms_max=max(ms), sparse_pass_ms=sparse,
                      median_over_sparse=float(np.median(ms)) / sparse, max_over_sparse=max(ms) / sparse, bar=bar, launches_rerun=rerun))
    t.close()


def section_tile(a):
    n, nl, bits = a.small_rows, 65536, 1024
    t = make(n, bits, TILE)
    with knob(None):
        left = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, n, nl, 0)
    t.join(left, 0.7)
    for rep in range(2):
        st = {}
        t.join(left, 0.7, stats=st)
        pps = nl * n / (st["tile_ms"] * 1e-3)
        ceil = 1024 * st["clock_mhz"] * 1e6 / 8.8 * 64 / (bits // 32)
        emit(dict(section="tile", rows=n, left_rows=nl, bits=bits, cutoff=0.7, rep=rep, pairs_listed=int(st["pairs"]),
                  launches=int(st["tile_launches"]), launches_rerun=int(st["launches_rerun"]), tile_ms=st["tile_ms"],
                  mean_launch_ms=st["tile_ms"] / st["tile_launches"], csr_ms=st["csr_ms"], d2h_ms=st["d2h_ms"],
                  call_ms=st["wall_ms"], clock_mhz=st["clock_mhz"], pairs_per_s=pps, ceiling_pairs_per_s=ceil,
                  fraction_of_ceiling=pps / ceil, bar_fraction=0.7, whole_over_tile=st["wall_ms"] / st["tile_ms"], bar_whole=1.25))
    t.close()
    left.close()


def section_crossover(a):
    shapes = [(a.small_rows, 1024), (a.rows, 1024), (a.small_rows * 8, 128), (a.small_rows // 2, 2048)]
    for n, bits in shapes:
        left = left_rows(n, bits, 256)
        times = {}
        for route in (STREAM, TILE):
            t = make(n, bits, route)
            t.join(left[:1], 0.7)
            for nl in (1, 2, 4, 8, 16, 32, 64, 128, 256):
                best = None
                for rep in range(3):
                    st = {}
                    t.join(left[:nl], 0.7, stats=st)
                    ms = st["stream_ms"] + st["tile_ms"]
                    best = ms if best is None else min(best, ms)
                times[(route, nl)] = best
            t.close()
        td = make(n, bits, None)
        for nl in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            st = {}
            td.join(left[:nl], 0.7, stats=st)
            took = "stream" if st["rows_streamed"] else "tile"
            s, tl = times[(STREAM, nl)], times[(TILE, nl)]
            mine = s if took == "stream" else tl
            emit(dict(section="crossover", rows=n, bits=bits, left_rows=nl, stream_ms=s, tile_ms=tl, default_takes=took,
                      default_over_faster=mine / min(s, tl), bar=1.15))
        td.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="stream,dense,tile,crossover")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--small-rows", type=int, default=1_000_000)
    a = ap.parse_args()
    a.sections = a.sections.split(",")
    if "stream" in a.sections or "dense" in a.sections:
        section_stream(a)
    if "tile" in a.sections:
        section_tile(a)
    if "crossover" in a.sections:
        section_crossover(a)


if __name__ == "__main__":
    main()
