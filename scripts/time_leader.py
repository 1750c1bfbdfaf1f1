"""Time gsim_db_leader on generated Morgan-shaped tables and put it beside the library's other two ways to organise a table
(DESIGN.md section 14).

    python scripts/time_leader.py [--bits 1024] [--rows 1000000] [--cutoffs 0.3,0.5,0.7] [--big-rows 100000000] [--big-cap 10000]
                                  [--rounds 64,128,256,512,1024] [--maxmin-max-picks 20000] [--timeout 600] [--json out.json]

One child process per configuration, each under its own timeout; the run stops at the first child that fails.  In this order:
  leader      rows x cutoffs without a cap; --big-rows at cutoff 0.5 with max_leaders = --big-cap; then the round-size sweep
              (GSIM_LEADER_ROUND) at --rows and cutoff 0.5
  maxmin      gsim_db_maxmin on the same table with as many picks as the leader call made leaders (more than --maxmin-max-picks:
              that many are timed and the figure is scaled, and says so)
  butina      gsim_db_neighbors + gsim_butina on the same table and cutoff, --rows only, highest cutoff first (the graph grows as the
              cutoff falls)
Per leader configuration: leaders, rounds, pairs; pairs over N x leaders (1.0: nothing ever left the list); the pass's pair rate
= pairs / (kernel_ms - resolve_ms - compact_ms), to be read against group_scan_kernel's at the same width
(profiles/grp_time_group.txt); and the shares of the call's wall time: resolve, compaction, host (wall - kernel - d2h: the
per-round control reads and the set-up)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x1EADE2


def child(cfg):
    import numpy as np
    from gpusimilarity_amd import capi
    t = capi.Table(cfg["bits"]).generate(SEED, capi.SYNTH_MORGAN, 0, cfg["rows"], 0)
    n = cfg["rows"]
    rec = dict(cfg)
    if cfg["what"] == "leader":
        t.leader(cfg["cutoff"], max_leaders=min(8, n), assign=False)  # warm-up: loads the kernels
        best = None
        for _ in range(cfg["reps"]):
            leaders, _, _, st = t.leader(cfg["cutoff"], max_leaders=cfg.get("cap"), assign=False)
            if best is None or st["wall_ms"] < best["wall_ms"]:
                best = st
        st = best
        pass_ms = st["kernel_ms"] - st["resolve_ms"] - st["compact_ms"]
        rec.update({k: (int(v) if isinstance(v, int) else v) for k, v in st.items()})
        rec.update(pairs_over_n_leaders=st["pairs"] / (n * max(st["leaders"], 1)), pass_ms=pass_ms,
                   pass_pairs_per_s=st["pairs"] / (pass_ms * 1e-3) if pass_ms > 0 else 0.0,
                   share_resolve=st["resolve_ms"] / st["wall_ms"], share_compact=st["compact_ms"] / st["wall_ms"],
                   share_host=(st["wall_ms"] - st["kernel_ms"] - st["d2h_ms"]) / st["wall_ms"])
    elif cfg["what"] == "maxmin":
        picks = min(cfg["picks"], cfg["max_picks"], n)
        t.maxmin(min(8, n))
        st = {}
        t.maxmin(picks, stats=st)
        scale = cfg["picks"] / max(st["picks"], 1)
        rec.update(timed_picks=int(st["picks"]), kernel_ms=st["kernel_ms"], wall_ms=st["wall_ms"], scaled=scale > 1.0,
                   wall_ms_for_all_picks=st["wall_ms"] * max(scale, 1.0))
    else:
        st = {}
        w0 = time.perf_counter()
        indptr, indices, _ = t.neighbors(cfg["cutoff"], stats=st)
        w1 = time.perf_counter()
        cluster_of, centroids = capi.butina(indptr, indices)
        w2 = time.perf_counter()
        rec.update(edges=int(len(indices)), clusters=int(len(centroids)), neighbors_ms=(w1 - w0) * 1e3, butina_ms=(w2 - w1) * 1e3,
                   tile_ms=st["tile_ms"], total_ms=(w2 - w0) * 1e3)
    t.close()
    print(json.dumps(rec), flush=True)


def run(cfg, timeout, env=None):
    e = dict(os.environ)
    e.update(env or {})
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(cfg)], capture_output=True, text=True,
                           timeout=timeout, env=e)
    except subprocess.TimeoutExpired:
        print("FAILED (timeout %d s): %s" % (timeout, json.dumps(cfg)), flush=True)
        return None
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        print("FAILED (exit %d): %s\n%s" % (p.returncode, json.dumps(cfg), p.stderr[-2000:]), flush=True)
        return None
    print(lines[-1], flush=True)
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cutoffs", default="0.3,0.5,0.7")
    ap.add_argument("--big-rows", type=int, default=100_000_000)
    ap.add_argument("--big-cap", type=int, default=10_000)
    ap.add_argument("--rounds", default="64,128,256,512,1024")
    ap.add_argument("--maxmin-max-picks", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.child:
        child(json.loads(a.child))
        return 0
    cutoffs = [float(c) for c in a.cutoffs.split(",") if c]
    out, leaders = [], {}

    def step(cfg, env=None):
        rec = run(cfg, a.timeout, env)
        if rec is None:
            if a.json:
                json.dump(out, open(a.json, "w"), indent=1)
            sys.exit(1)  # the first failure ends the run
        out.append(rec)
        return rec

    for c in cutoffs:
        leaders[(a.rows, c)] = step(dict(what="leader", bits=a.bits, rows=a.rows, cutoff=c, reps=a.reps))["leaders"]
    if a.big_rows:
        leaders[(a.big_rows, 0.5)] = step(dict(what="leader", bits=a.bits, rows=a.big_rows, cutoff=0.5, cap=a.big_cap, reps=a.reps))["leaders"]
    for b in [int(x) for x in a.rounds.split(",") if x]:
        step(dict(what="leader", bits=a.bits, rows=a.rows, cutoff=0.5, reps=a.reps, round=b), {"GSIM_LEADER_ROUND": str(b)})
    for (rows, c), n in leaders.items():
        step(dict(what="maxmin", bits=a.bits, rows=rows, cutoff=c, picks=int(n), max_picks=a.maxmin_max_picks))
    for c in sorted(cutoffs, reverse=True):
        step(dict(what="butina", bits=a.bits, rows=a.rows, cutoff=c))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
