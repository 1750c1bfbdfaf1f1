"""Time gsim_db_scores_device (HIP events inside the library) on synthetic tables made on the device, beside the fastest way the
library could evaluate the same pairs before: the join's tile route at a cutoff that keeps nothing, on the same rectangle in the
same run.

    python scripts/time_scores.py [--bits 256,1024,2048] [--rows 1000000] [--left 16384] [--cols 65536] [--host-left 4096] [--json FILE]

Per width: GSIM_SYNTH_SPARSE rows, LEFT left rows (a table of another seed) against the COLS-row range [COL0, COL0 + COLS) of a
ROWS-row table, written into a torch tensor (LEFT x COLS x 4 bytes: 4 GiB at the defaults): kernel_ms (best of --reps), pairs/s
and the clock the kernel itself measured.  The yardstick is gsim_db_join of the same left rows against a table that holds exactly
that range (generated from the same seed and first row), tile route (GSIM_JOIN_STREAM_MAX_ROWS=0), cutoff 1.0 -- i.i.d. rows of
different seeds: nothing is kept, nothing is divided or stored -- gsim_join_stats.tile_ms.  Two derived ceilings beside them: 4 bytes
per pair at the 8 TB/s write peak (2.0e12 pairs/s), and the MFMA issue time of WP / 2 instructions of 32 cycles per 32 x 32 tile on
1024 SIMDs at the measured clock.  Then one host-output call of HOST_LEFT x COLS, to show how much of that call is the copy."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

SEED, LEFT_SEED = 0xC0FFEE, 0x5C02E5
WRITE_PEAK = 8.0e12  # bytes/s
SIMDS, MFMA_CYCLES = 1024, 32
OUT = []


def emit(**rec):
    print(json.dumps(rec), flush=True)
    OUT.append(rec)


def generate(bits, seed, first, n, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return capi.Table(bits).generate(seed, capi.SYNTH_SPARSE, first, n, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="256,1024,2048")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--left", type=int, default=16384)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--col0", type=int, default=500_000)
    ap.add_argument("--host-left", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    c0, c1 = a.col0, a.col0 + a.cols
    out = torch.empty((a.left, a.cols), dtype=torch.float32, device="cuda:0")
    for bits in [int(x) for x in a.bits.split(",")]:
        wp = (bits // 32 + 7) // 8 * 8
        table = generate(bits, SEED, 0, a.rows)
        left = generate(bits, LEFT_SEED, 0, a.left)
        window = generate(bits, SEED, c0, a.cols, GSIM_JOIN_STREAM_MAX_ROWS=0)  # the rows [c0, c1) of `table`
        assert (window.row(0) == table.row(c0)).all() and (window.row(a.cols - 1) == table.row(c1 - 1)).all()
        pairs = a.left * a.cols
        # both kernels alternate; the first round is the warm-up
        best, join_best = None, None
        for rep in range(a.reps + 1):
            st, js = {}, {}
            table.scores(left, col_begin=c0, col_end=c1, out_ptr=out.data_ptr(), stats=st)
            window.join(left, 1.0, stats=js)
            assert js["pairs"] == 0 and js["rows_tiled"] == a.left, js
            if rep and (best is None or st["kernel_ms"] < best["kernel_ms"]):
                best = st
            if rep and (join_best is None or js["tile_ms"] < join_best["tile_ms"]):
                join_best = js
        rate = pairs / (best["kernel_ms"] * 1e-3)
        join_rate = pairs / (join_best["tile_ms"] * 1e-3)
        write_ceiling = WRITE_PEAK / 4
        mfma_ceiling = SIMDS * best["clock_mhz"] * 1e6 * 1024 / (wp / 2 * MFMA_CYCLES)
        emit(what="scores_device", bits=bits, rows=a.rows, left_rows=a.left, cols=a.cols, pairs=pairs, kernel_ms=best["kernel_ms"],
             prepare_ms=best["prepare_ms"], call_ms=best["wall_ms"], launches=int(best["launches"]), clock_mhz=best["clock_mhz"],
             pairs_per_s=rate, join_tile_ms=join_best["tile_ms"], join_tile_launches=int(join_best["tile_launches"]),
             join_clock_mhz=join_best["clock_mhz"], join_pairs_per_s=join_rate, rate_over_join_tiles=rate / join_rate,
             write_ceiling_pairs_per_s=write_ceiling, mfma_ceiling_pairs_per_s=mfma_ceiling,
             fraction_of_lower_ceiling=rate / min(write_ceiling, mfma_ceiling), lower_ceiling="write" if write_ceiling < mfma_ceiling else "mfma",
             written_gb_per_s=rate * 4e-9)
        st = {}
        host = table.scores(left, row_end=min(a.host_left, a.left), col_begin=c0, col_end=c1, stats=st)
        check = out[:host.shape[0]].cpu().numpy()
        assert host.tobytes() == check.tobytes(), "host output == device output"
        emit(what="scores_host", bits=bits, left_rows=host.shape[0], cols=a.cols, bytes=host.nbytes, call_ms=st["wall_ms"], kernel_ms=st["kernel_ms"],
             d2h_ms=st["d2h_ms"], prepare_ms=st["prepare_ms"], slabs=int(st["slabs"]), launches=int(st["launches"]),
             copy_share=st["d2h_ms"] / st["wall_ms"], d2h_gb_per_s=host.nbytes / (st["d2h_ms"] * 1e-3) * 1e-9)
        del host, check
        for t in (table, left, window):
            t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(OUT, f, indent=1)


if __name__ == "__main__":
    main()
