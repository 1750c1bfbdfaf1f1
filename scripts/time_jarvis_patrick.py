"""Time gsim_db_jarvis_patrick (HIP events inside the library: the k-NN fold, the list sort, the link pass with its flatten, the
labelling, D2H) on synthetic tables, beside the route that existed before it on the same table in the same run: gsim_db_knn, its CSR
copied to the host, and the host function gsim_jarvis_patrick on it.

    python scripts/time_jarvis_patrick.py [--rows 100000,1000000] [--bits 1024] [--kind morgan] [--cases 16:8,128:64] [--reps 1]
                                          [--out profiles/jarvis_patrick_time.txt]

Per table and case k:kmin, at the smallest positive cutoff: fold, sort, link and label ms; the link pass's entries/s and the bytes/s
it gathers -- every entry loads the k words of its neighbour's sorted list, entries x k x 4 bytes, set beside the 8 TB/s of the
device's memory --; the share of the device call's kernel time that the new passes (sort + link + label) take; and the host route's
three parts (gsim_db_knn's wall time, which includes its D2H, and the host clustering) with a byte comparison of the two results."""
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
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--kind", default="morgan")
    ap.add_argument("--cases", default="16:8,128:64")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jarvis_patrick_time.txt"))
    a = ap.parse_args()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    # warm-up on a small table: loads every kernel the timed calls use
    w = capi.Table(a.bits).generate(0xC0FFEE, KINDS[a.kind], 0, 4096, 0)
    for k, kmin in cases:
        w.jarvis_patrick(k, kmin, TINY)
        w.knn(k, TINY)
    w.close()
    for rows in (int(r) for r in a.rows.split(",")):
        t = capi.Table(a.bits).generate(0xC0FFEE, KINDS[a.kind], 0, rows, 0)
        name = "%s %d x %d" % (a.kind, rows, a.bits)
        for k, kmin in cases:
            for rep in range(a.reps):
                levels, st = t.jarvis_patrick(k, kmin, TINY)
                cluster_of, first_row, sizes = levels[0]
                new_ms = st["sort_ms"] + st["link_ms"] + st["label_ms"]
                link_s = st["link_ms"] * 1e-3
                gathered = st["entries"] * k * 4
                emit(call="jarvis_patrick", table=name, k=k, kmin=kmin, cutoff=TINY, rep=rep, entries=st["entries"],
                     mutual_entries=st["mutual_entries"], links=st["links"][0], unions=st["unions"], cas_failed=st["cas_failed"],
                     clusters=len(first_row), clusters_of_two_or_more=int((sizes >= 2).sum()), largest=int(sizes.max()),
                     knn_ms=st["knn_ms"], sort_ms=st["sort_ms"], link_ms=st["link_ms"], label_ms=st["label_ms"], d2h_ms=st["d2h_ms"],
                     wall_ms=st["wall_ms"], launches=st["launches"], clock_mhz=st["clock_mhz"],
                     link_entries_per_s=st["entries"] / link_s, link_gathered_bytes_per_s=gathered / link_s,
                     link_fraction_of_8TBps=gathered / link_s / HBM_BYTES_PER_S, new_passes_ms=new_ms,
                     new_passes_share_of_kernel_time=new_ms / (new_ms + st["knn_ms"]))
                ks = {}
                t0 = time.perf_counter()
                indptr, indices, _ = t.knn(k, TINY, stats=ks)
                t1 = time.perf_counter()
                host = capi.jarvis_patrick(indptr, indices, kmin)[0]
                t2 = time.perf_counter()
                emit(call="knn + host jarvis_patrick", table=name, k=k, kmin=kmin, cutoff=TINY, rep=rep, knn_kernel_ms=ks["kernel_ms"],
                     knn_csr_ms=ks["csr_ms"], knn_d2h_ms=ks["d2h_ms"], knn_wall_ms=(t1 - t0) * 1e3, host_ms=(t2 - t1) * 1e3,
                     route_ms=(t2 - t0) * 1e3, device_call_wall_ms=st["wall_ms"], route_over_device_call=(t2 - t0) * 1e3 / st["wall_ms"],
                     same_bytes=bool(host[0].tobytes() == cluster_of.tobytes() and host[1].tobytes() == first_row.tobytes()
                                     and host[2].tobytes() == sizes.tobytes()))
                del indptr, indices, host
        t.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
