"""Time gsim_db_dbscan (HIP events inside the library: the degree pass, the link pass with its flatten launches, labelling, D2H) on
synthetic tables, beside one gsim_db_components pass on the same table at the same cutoff in the same run, and report pairs/s of each
pass against the VALU engine's ceiling (DESIGN.md sections 9, 18 and 26).

    python scripts/time_dbscan.py [--rows 1000000] [--bits 1024] [--min-pts 5] [--kinds sparse,morgan] [--reps 3]
                                  [--sparse-cutoffs 0.7,0.05] [--morgan-cutoffs 0.7,0.3] [--out profiles/dbscan_time.txt]

Per kind and cutoff -- the first of a kind's cutoffs is meant to leave mostly noise, the second to form a giant cluster; the census
of every run is in its line -- (1) gsim_db_dbscan with the link pass's wave-level skip on (the default), (2) the same with
GSIM_DBSCAN_SKIP=0 on a second handle over the same generated rows, (3) gsim_db_components at that cutoff.  No threshold is set: two
pair passes should cost about two components passes, and the summary lines give the ratio.
Ceiling: as scripts/time_components.py -- 8.8 cycles per wave64 v_and + v_bcnt pair per SIMD, 1024 SIMDs, 64 pairs per instruction
pair, rows padded to WP words -- at the clock the tile kernels themselves measured (clock_mhz)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpusimilarity_amd import capi  # noqa: E402

KINDS = {"sparse": capi.SYNTH_SPARSE, "dense": capi.SYNTH_DENSE, "morgan": capi.SYNTH_MORGAN}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--min-pts", type=int, default=5)
    ap.add_argument("--kinds", default="sparse,morgan")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sparse-cutoffs", default="0.7,0.05")
    ap.add_argument("--morgan-cutoffs", default="0.7,0.3")
    ap.add_argument("--dense-cutoffs", default="0.7,0.3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_time.txt"))
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

    def make(kind, skip):
        old = os.environ.get("GSIM_DBSCAN_SKIP")
        os.environ["GSIM_DBSCAN_SKIP"] = "1" if skip else "0"  # (read once per handle, when it is created)
        try:
            return capi.Table(a.bits).generate(0xC0FFEE, KINDS[kind], 0, a.rows, 0)
        finally:
            if old is None:
                del os.environ["GSIM_DBSCAN_SKIP"]
            else:
                os.environ["GSIM_DBSCAN_SKIP"] = old

    def dbscan(t, what, cutoff, skip):
        t.dbscan(cutoff, a.min_pts, degree=False, anchor=False, first_row=False, sizes=False)  # warm-up: loads the kernels
        best = None
        for rep in range(a.reps):
            out = t.dbscan(cutoff, a.min_pts)
            sizes, st = out[4], out[5]
            top = ceiling(st["clock_mhz"]) if st["clock_mhz"] else None
            count_rate, link_rate = st["pairs"] / (st["count_ms"] * 1e-3), st["pairs"] / (st["link_ms"] * 1e-3)
            emit(call="dbscan", table=what, cutoff=cutoff, min_pts=a.min_pts, skip=int(skip), rep=rep, count_ms=st["count_ms"],
                 link_ms=st["link_ms"], label_ms=st["label_ms"], d2h_ms=st["d2h_ms"], wall_ms=st["wall_ms"],
                 launches_count=int(st["launches_count"]), launches_link=int(st["launches_link"]), kept=int(st["kept"]), cores=int(st["cores"]),
                 borders=int(st["borders"]), noise=int(st["noise"]), clusters=int(st["clusters"]), unions=int(st["unions"]),
                 cas_failed=int(st["cas_failed"]), largest=int(sizes.max()) if len(sizes) else 0, count_pairs_per_s=count_rate,
                 link_pairs_per_s=link_rate, clock_mhz=st["clock_mhz"], count_fraction_of_ceiling=count_rate / top if top else None,
                 link_fraction_of_ceiling=link_rate / top if top else None)
            if best is None or st["count_ms"] + st["link_ms"] < best[0] + best[1]:
                best = (st["count_ms"], st["link_ms"])
        return best

    def components(t, what, cutoff):
        t.components([cutoff], first_row=False, sizes=False)  # warm-up
        best = None
        for rep in range(a.reps):
            levels, st = t.components([cutoff])
            rate = st["pairs"] / (st["kernel_ms"] * 1e-3)
            emit(call="components", table=what, cutoff=cutoff, rep=rep, kernel_ms=st["kernel_ms"], label_ms=st["label_ms"], wall_ms=st["wall_ms"],
                 launches=int(st["launches"]), kept=int(st["kept"]), ncomponents=int(len(levels[0][1])), largest=int(levels[0][2].max()),
                 pairs_per_s=rate, clock_mhz=st["clock_mhz"], fraction_of_ceiling=rate / ceiling(st["clock_mhz"]) if st["clock_mhz"] else None)
            best = st["kernel_ms"] if best is None else min(best, st["kernel_ms"])
        return best

    for kind in a.kinds.split(","):
        what = "%s %d x %d" % (kind, a.rows, a.bits)
        t, t_noskip = make(kind, True), make(kind, False)
        for cutoff in [float(c) for c in getattr(a, kind + "_cutoffs").split(",")]:
            on = dbscan(t, what, cutoff, True)
            off = dbscan(t_noskip, what, cutoff, False)
            comp = components(t, what, cutoff)
            emit(summary=what, cutoff=cutoff, min_pts=a.min_pts, count_ms=on[0], link_ms=on[1], link_ms_without_skip=off[1],
                 components_kernel_ms=comp, count_over_components=on[0] / comp, link_over_components=on[1] / comp,
                 both_passes_over_two_components=(on[0] + on[1]) / (2 * comp), skip_gain=off[1] / on[1])
        t.close()
        t_noskip.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
