"""Time gsim_db_search_rows route by route on generated Morgan-shaped tables.

    python scripts/time_subset.py [--rows 100000000,1000000] [--bits 1024] [--k 1000] [--queries 8] [--reps 3] [--out FILE.json]

For every table size N and every set size N/2, N/10, N/100, N/1000, N/10 000, for a random and a contiguous set:
  stream_ms / gather_ms   per-query time of each route forced (GSIM_SUBSET_GATHER_MAX_PERMILLE = 0 / 1000): the call's wall time over
                          its queries, best of --reps calls (kernel_ms, HIP events inside the library, beside it)
  default_takes           the route a handle with the default knob picks, and what it costs against the faster forced route (bar 1.15)
  search_ms               gsim_db_search (k, one query at a time, GSIM_FUSED=0: the four-kernel pipeline) on the same handle's table
                          -- what the streaming route is held against at N/2 (bar 1.05)
  plain_ms                gsim_db_search on a plain generated table of `selected` rows (default knobs): what a copy of the set costs
  gather_ns_per_row       gather time per selected row, beside the plain scan's time per table row (scan_ns_per_row)"""
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
KNOB = "GSIM_SUBSET_GATHER_MAX_PERMILLE"
STREAM, GATHER = "0", "1000"


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


def make(n, bits, route, fused="0"):
    with env(**{KNOB: route, "GSIM_FUSED": fused}):
        return capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, n, 0)


def emit(rec, sink):
    print(json.dumps(rec), flush=True)
    sink.append(rec)


def search_ms(t, queries, k, reps):
    bufs = t.make_search_buffers(len(queries), k)
    t.search_timed_into(queries, k, bufs)  # warm-up: loads the kernels, allocates the scratch
    best = None
    for _ in range(reps):
        sec = t.search_timed_into(queries, k, bufs)
        ms = float(np.median(sec)) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def rows_ms(t, rs, queries, k, reps):
    """-> (wall ms per query, kernel ms per query, stats of the last call)"""
    t.search_rows(rs, queries[:1], k)
    wall = kern = None
    st = None
    for _ in range(reps):
        _, _, st = t.search_rows(rs, queries, k, stats=True)
        w, kk = st["wall_ms"] / len(queries), st["kernel_ms"] / len(queries)
        wall = w if wall is None else min(wall, w)
        kern = kk if kern is None else min(kern, kk)
    return wall, kern, st


def make_set(t, n, m, shape, rng):
    if shape == "contiguous":
        lo = (n - m) // 3
        return t.rowset(rows=np.arange(lo, lo + m, dtype=np.uint32))
    if 2 * m >= n:  # a random half: random words
        return t.rowset(bitmap=rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32))
    return t.rowset(rows=rng.integers(0, n, m, dtype=np.uint64).astype(np.uint32))  # (duplicates collapse: `selected` says what is left)


def run(n, a, sink):
    bits, k = a.bits, a.k
    queries = np.stack([capi.synth_row(SEED, capi.SYNTH_MORGAN, n + i, bits) for i in range(a.queries)])
    tables = {"stream": make(n, bits, STREAM), "gather": make(n, bits, GATHER), "default": make(n, bits, None)}
    scan = search_ms(tables["stream"], queries, k, a.reps)
    emit(dict(section="search", rows=n, bits=bits, k=k, fused=0, search_ms=scan, scan_ns_per_row=scan * 1e6 / n), sink)
    for div in (2, 10, 100, 1000, 10000):
        for shape in ("random", "contiguous"):
            m = n // div
            rec = dict(section="subset", rows=n, bits=bits, k=k, shape=shape, divisor=div)
            for name in ("stream", "gather"):
                rng = np.random.default_rng(div * 7 + 1)
                rs = make_set(tables[name], n, m, shape, rng)
                wall, kern, st = rows_ms(tables[name], rs, queries, k, a.reps)
                assert st["queries_" + name] == len(queries)
                rec["selected"] = int(st["selected"])
                rec[name + "_ms"], rec[name + "_kernel_ms"] = wall, kern
                rs.close()
            rs = make_set(tables["default"], n, m, shape, np.random.default_rng(div * 7 + 1))
            _, _, st = tables["default"].search_rows(rs, queries[:1], k, stats=True)
            rs.close()
            took = "gather" if st["queries_gather"] else "stream"
            sel = rec["selected"]
            plain = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, sel, 0)
            rec.update(default_takes=took, default_over_faster=rec[took + "_ms"] / min(rec["stream_ms"], rec["gather_ms"]), bar_default=1.15,
                       search_ms=scan, stream_over_search=rec["stream_ms"] / scan, bar_stream_at_half=1.05 if div == 2 and shape == "random" else None,
                       plain_ms=search_ms(plain, queries, min(k, sel), a.reps), gather_ns_per_row=rec["gather_ms"] * 1e6 / sel,
                       scan_ns_per_row=scan * 1e6 / n)
            plain.close()
            emit(rec, sink)
    for t in tables.values():
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000000,1000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sink = []
    for n in (int(x) for x in a.rows.split(",")):
        run(n, a, sink)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(sink, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
