"""Time gsim_db_assign, gsim_db_label_counts and gsim_db_kmeans (HIP events inside the library) beside the routes the library had
before them, in the same run.

    python scripts/time_kmeans.py [--rows 1000000] [--big-rows 100000000] [--bits 1024,2048] [--centres 1024,16384] [--reps 3]
                                  [--out profiles/kmeans_time.txt]

gsim_db_assign: per width and number of centres the assign kernel (kernel_ms, pairs/s, clock, the fraction of section 17's MFMA
ceiling) and, ALTERNATING with it repetition by repetition, gsim_db_scores_device on the same rectangle (kernel_ms) plus torch's
arg-max over that tensor (torch events).  The rectangle of the scores route is cut into column blocks that fit --scores-bytes of
device memory; its times are summed.  At --big-rows one line of gsim_db_assign alone with the first number of centres.
gsim_db_label_counts: Morgan rows of the first width, uniform labels over 1000 and 100 000 labels: sort_ms, kernel_ms, the fraction
of 8 TB/s of the counting kernel, beside one plain gsim_db_bit_counts pass over the table (the read bound) and the loop the library
offered before: gsim_db_bit_counts over a row set per label, timed on 20 labels and SCALED to L (an extrapolation, marked as such).
gsim_db_kmeans: --rows rows, 1000 centres (rows of the table), 5 iterations: the assign / counts / update split per iteration."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

HBM = 8e12
SEED = 0xC0FFEE
MFMA_CYCLES = 32  # of one v_mfma_scale_f32_32x32x64_f8f6f4 (scripts/time_scores.py)


def mfma_ceiling_pairs_per_s(words, cus, mhz):
    """section 17's ceiling: a 32 x 32 tile (1024 pairs) takes words / 2 MFMAs (four per 256-bit group) on one of the 4 x CUs SIMDs"""
    wp = (words + 7) // 8 * 8
    return 4 * cus * mhz * 1e6 * 1024 / (wp / 2 * MFMA_CYCLES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--big-rows", type=int, default=100000000)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--centres", default="1024,16384")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scores-bytes", type=int, default=8 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_time.txt"))
    a = ap.parse_args()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# scripts/time_kmeans.py: %s, %d CUs; best of %d repetitions after a warm-up; kernel ms by HIP events" % (torch.cuda.get_device_name(0), cus, a.reps))
    widths = [int(b) for b in a.bits.split(",")]
    ms_ = [int(m) for m in a.centres.split(",")]

    # ---- gsim_db_assign against gsim_db_scores_device + torch arg-max ----
    say("## assign: rows bits centres | assign kernel_ms pairs/s clock_mhz of_mfma_ceiling | scores kernel_ms argmax_ms | assign/scores")
    for bits in widths:
        t = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, a.rows, 0)
        for m in ms_:
            cen_t = capi.Table(bits).generate(SEED + 1, capi.SYNTH_MORGAN, 0, m, 0)
            cen = np.stack([cen_t.row(i) for i in range(m)])
            cols = max(min(a.rows, a.scores_bytes // (4 * m)) // 128 * 128, 128)
            out = torch.empty((m, cols), dtype=torch.float32, device="cuda:0")
            best_a, best_s, best_x, st_a = 1e30, 1e30, 1e30, None
            for rep in range(a.reps + 1):
                st = {}
                t.assign(cen, stats=st)
                s_ms, x_ms = 0.0, 0.0
                for c0 in range(0, a.rows, cols):
                    c1 = min(c0 + cols, a.rows)
                    ss = {}
                    t.scores(cen_t, col_begin=c0, col_end=c1, out_ptr=out.data_ptr(), ld=cols, stats=ss)
                    s_ms += ss["kernel_ms"]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    am = torch.argmax(out[:, :c1 - c0], dim=0)
                    e1.record()
                    torch.cuda.synchronize()
                    x_ms += e0.elapsed_time(e1)
                    del am
                if rep == 0:  # (the warm-up)
                    continue
                if st["kernel_ms"] < best_a:
                    best_a, st_a = st["kernel_ms"], st
                best_s, best_x = min(best_s, s_ms), min(best_x, x_ms)
            pps = st_a["pairs"] / (best_a * 1e-3)
            say("assign %d %d %d | %.3f %.3e %.0f %.3f | %.3f %.3f | %.3f" % (
                a.rows, bits, m, best_a, pps, st_a["clock_mhz"], pps / mfma_ceiling_pairs_per_s(bits // 32, cus, st_a["clock_mhz"]), best_s, best_x,
                best_a / best_s))
            del out
            cen_t.close()
        t.close()

    # ---- gsim_db_label_counts against one bit_counts pass and the loop over row sets ----
    bits = widths[0]
    say("## label_counts: rows bits labels | sort_ms kernel_ms of_8TB/s | bit_counts_ms ratio | loop over 20 row sets ms, scaled to L (extrapolated) ms")
    for rows in (a.rows, a.big_rows):
        if rows <= 0:
            continue
        try:
            t = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, rows, 0)
        except capi.GsimError as e:
            say("label_counts %d %d: table not made (%s)" % (rows, bits, e))
            continue
        if rows == a.big_rows:
            cen_t = capi.Table(bits).generate(SEED + 1, capi.SYNTH_MORGAN, 0, ms_[0], 0)
            cen = np.stack([cen_t.row(i) for i in range(ms_[0])])
            best, st_a = 1e30, None
            for rep in range(2):
                st = {}
                t.assign(cen, stats=st)
                if st["kernel_ms"] < best:
                    best, st_a = st["kernel_ms"], st
            pps = st_a["pairs"] / (best * 1e-3)
            say("assign %d %d %d | %.3f %.3e %.0f %.3f | - - | - (launches %d, prepare_ms %.3f, d2h_ms %.3f)" % (
                rows, bits, ms_[0], best, pps, st_a["clock_mhz"], pps / mfma_ceiling_pairs_per_s(bits // 32, cus, st_a["clock_mhz"]),
                st_a["launches"], st_a["prepare_ms"], st_a["d2h_ms"]))
            cen_t.close()
        rng = np.random.default_rng(1)
        for L in (1000, 100000):
            labels = rng.integers(0, L, rows, dtype=np.uint32)
            best = None
            for rep in range(a.reps + 1):
                st = {}
                t.label_counts(labels, L, stats=st)
                if rep and (best is None or st["kernel_ms"] < best["kernel_ms"]):
                    best = st
            bc = 1e30
            for rep in range(a.reps + 1):
                st = {}
                t.bit_counts(stats=st)
                if rep:
                    bc = min(bc, st["kernel_ms"])
            t0 = time.perf_counter()
            for l in range(20):
                rs = t.rowset(rows=np.flatnonzero(labels == l).astype(np.uint32))
                t.bit_counts(rowset=rs)
                rs.close()
            loop_ms = (time.perf_counter() - t0) * 1e3
            say("label_counts %d %d %d | %.3f %.3f %.3f | %.3f %.2f | %.1f %.0f" % (
                rows, bits, L, best["sort_ms"], best["kernel_ms"], rows * (bits / 8) / (best["kernel_ms"] * 1e-3) / HBM, bc, best["kernel_ms"] / bc,
                loop_ms, loop_ms * L / 20))
            del labels
        t.close()

    # ---- gsim_db_kmeans ----
    say("## kmeans: rows bits centres | iterations converged changed_last | assign_ms counts_ms update_ms wall_ms | per iteration")
    t = capi.Table(bits).generate(SEED, capi.SYNTH_MORGAN, 0, a.rows, 0)
    m = 1000
    init = np.stack([t.row(i * (a.rows // m)) for i in range(m)])
    for rep in range(2):
        _, _, _, _, st = t.kmeans(init, 5)
    it = st["iterations"]
    say("kmeans %d %d %d | %d %d %d | %.3f %.3f %.3f %.3f | %.3f %.3f %.3f" % (
        a.rows, bits, m, it, st["converged"], st["changed_last"], st["assign_ms"], st["counts_ms"], st["update_ms"], st["wall_ms"],
        st["assign_ms"] / it, st["counts_ms"] / max(it - 1, 1), st["update_ms"] / it))
    t.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
