"""Time gsim_db_components (HIP events inside the library: tile + flatten launches, labelling, D2H) on synthetic tables, against
gsim_db_neighbors' tile kernel on the same table in the same run, and report pairs/s against the VALU engine's ceiling
(DESIGN.md sections 9 and 18).

    python scripts/time_components.py [--rows 1000000] [--bits 1024] [--cutoff 0.7] [--kinds sparse,morgan] [--reps 3]
                                      [--identical-rows 40000] [--out profiles/components_time_1M.txt]

Per kind: (1) one level at --cutoff, with gsim_db_neighbors at the same cutoff; (2) eight levels 0.3 ... 1.0 against one level at 0.3;
then (3) --identical-rows identical rows at cutoff 1.0 (every pair kept: the root cache's case) against gsim_db_neighbors there.
Ceiling: as scripts/time_neighbors.py -- 8.8 cycles per wave64 v_and + v_bcnt pair per SIMD, 1024 SIMDs, 64 pairs per instruction
pair, rows padded to WP words -- at the clock the tile kernel itself measured (clock_mhz)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpusimilarity_amd import capi  # noqa: E402

KINDS = {"sparse": capi.SYNTH_SPARSE, "dense": capi.SYNTH_DENSE, "morgan": capi.SYNTH_MORGAN}
LEVELS = [0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--cutoff", type=float, default=0.7)
    ap.add_argument("--kinds", default="sparse,morgan")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--identical-rows", type=int, default=40_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_time_1M.txt"))
    a = ap.parse_args()
    W = a.bits // 32
    wp = 4
    while wp < W:
        wp *= 2
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def ceiling(mhz):
        return 1024 * mhz * 1e6 / 8.8 * 64 / wp  # pairs/s at wp words per row

    def neighbours(t, what, cutoff, reps):
        t.neighbors(cutoff)  # warm-up: sizes the pair buffer, loads the kernels
        ms = []
        for rep in range(reps):
            st = {}
            t.neighbors(cutoff, stats=st)
            ms.append(st["tile_ms"])
            emit(call="neighbors", table=what, cutoff=cutoff, rep=rep, tile_ms=st["tile_ms"], launches=int(st["launches"]),
                 launches_rerun=int(st["launches_rerun"]), pairs_found=int(st["pairs"]), clock_mhz=st["clock_mhz"])
        return ms

    def components(t, what, cutoffs):
        t.components(cutoffs, first_row=False, sizes=False)  # warm-up: loads the kernels
        best = None
        for rep in range(a.reps):
            levels, st = t.components(cutoffs)
            rate = st["pairs"] / (st["kernel_ms"] * 1e-3)
            emit(call="components", table=what, cutoffs=cutoffs, rep=rep, kernel_ms=st["kernel_ms"], label_ms=st["label_ms"],
                 d2h_ms=st["d2h_ms"], wall_ms=st["wall_ms"], wall_over_kernel=st["wall_ms"] / st["kernel_ms"], launches=int(st["launches"]),
                 kept=int(st["kept"]), unions=int(st["unions"]), cas_failed=int(st["cas_failed"]),
                 ncomponents=[int(len(lv[1])) for lv in levels], largest=[int(lv[2].max()) for lv in levels], pairs_per_s=rate,
                 clock_mhz=st["clock_mhz"], fraction_of_ceiling=rate / ceiling(st["clock_mhz"]) if st["clock_mhz"] else None)
            best = st["kernel_ms"] if best is None else min(best, st["kernel_ms"])
        return best

    for kind in a.kinds.split(","):
        what = "%s %d x %d" % (kind, a.rows, a.bits)
        t = capi.Table(a.bits).generate(0xC0FFEE, KINDS[kind], 0, a.rows, 0)
        nb = neighbours(t, what, a.cutoff, a.reps)
        one = components(t, what, [a.cutoff])
        emit(summary=what, cutoff=a.cutoff, components_kernel_ms=one, neighbors_tile_ms=nb, ratio_to_best_neighbors=one / min(nb),
             neighbors_spread=max(nb) / min(nb))
        loosest = components(t, what, LEVELS[:1])
        eight = components(t, what, LEVELS)
        emit(summary=what, levels=LEVELS, eight_levels_kernel_ms=eight, one_level_kernel_ms=loosest, eight_over_one=eight / loosest)
        t.close()
    if a.identical_rows:
        n = a.identical_rows
        what = "identical %d x %d" % (n, a.bits)
        row = capi.synth_row(0xC0FFEE, KINDS["morgan"], 0, a.bits)
        t = capi.Table(a.bits).add_rows(np.tile(row, (n, 1))).finalize(0, 1)
        nb = neighbours(t, what, 1.0, min(a.reps, 2))  # (13 GB of CSR come back to the host per call)
        one = components(t, what, [1.0])
        emit(summary=what, cutoff=1.0, components_kernel_ms=one, neighbors_tile_ms=nb, ratio_to_best_neighbors=one / min(nb))
        t.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
