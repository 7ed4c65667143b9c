"""Times vrl_realign (-rq / -rt, include/vcfdist_realign.h) on callsets made from the synthetic workloads of bench.py: the query haps
of wgs_synth (1 M superclusters) and of one joint_synth slice (100 k), gap-clustered (-c gap 50).  Per workload: clusters, records,
kernel time of each pass (job list, pass 1, pass 2, backtracks), host time (merge + left_shift), wall time, clusters/s, rounds and
kept clusters; beside it the CPU model (tests/realign_model.py) on 16 processes over a slice of the clusters (--cpu-clusters), as
clusters/s.  One JSON line per workload; --out also writes them to a file.

    python tools/realign_bench.py [--workloads wgs_synth,joint_synth] [--reps 2] [--cpu-clusters 20000] [--out FILE]"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"wgs_synth": 1_000_000, "joint_synth": 100_000}
COLS = ("pos", "rlen", "type", "ref_len", "alt_len", "ref_off", "alt_off", "pool", "var_qual", "phase_set")


def haps_of(v, slot):
    """per contig: the slot's variants as a callset hap (positions are contig-relative) and the contig"""
    out = []
    for c in range(len(v.ctg_off) - 1):
        scs = np.nonzero(v.sc_ctg == c)[0]
        if len(scs) == 0:
            continue
        a, b = int(v.var_off[slot][scs[0]]), int(v.var_off[slot][scs[-1] + 1])
        h = dict(pos=v.var_pos[slot][a:b].copy(), type=v.var_type[slot][a:b].copy(), ref_len=v.var_ref_len[slot][a:b].copy(),
                 alt_len=v.var_alt_len[slot][a:b].copy(), ref_off=v.var_ref_off[slot][a:b].copy(), alt_off=v.var_alt_off[slot][a:b].copy(),
                 pool=v.allele_pool[slot], var_qual=v.var_qual[slot][a:b].copy(), phase_set=np.zeros(b - a, np.int32))
        h["rlen"] = h["ref_len"].copy()
        out.append((h, v.ctg_seq[v.ctg_off[c]:v.ctg_off[c + 1]]))
    return out


def _cpu_part(arg):
    """a worker (spawned: it never opens the GPU) runs the model over clusters [lo, hi) of the saved callset"""
    path, lo, hi = arg
    import realign_model as RM
    z = np.load(path)
    hap = {k: z[k] for k in COLS}
    seq = bytes(z["seq"]).decode()
    vb = z["var_beg"]
    t = time.perf_counter()
    for c in range(lo, hi):
        RM.realign_cluster(seq, hap, int(vb[c]), int(vb[c + 1]))
    return hi - lo, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="wgs_synth,joint_synth")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cpu-clusters", type=int, default=20000, help="clusters the CPU model runs on (0: none)")
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    import distance_helpers as DH
    from vcfdist_amd import api, cluster as K
    DH.model()                  # compiled once, before the workers start
    lines = []
    for w in args.workloads.split(","):
        syn = bench.make_workload(api, SIZES[w], args.seed, w)
        v = syn.variants()
        work = []
        for h, seq in haps_of(v, 0):
            cl = K.simple_cluster(K.Hap(h["pos"], h["rlen"], h["type"], h["ref_len"], h["alt_len"]), 0, 50, 10)
            work.append((h, cl, seq))
        runs = []
        for _ in range(args.reps):
            tot = dict(n_clusters=0, n_records=0, n_kept=0, n_limit=0, n_error=0, n_edge=0, n_rounds=0, n_hist_rounds=0, arena_peak_bytes=0,
                       ms_upload=0.0, ms_jobs=0.0, ms_score=0.0, ms_hist=0.0, ms_back=0.0, ms_host=0.0, ms_call=0.0)
            t = time.perf_counter()
            for h, cl, seq in work:
                _, _, i = api.realign(h, cl, seq)
                for k in ("n_clusters", "n_records", "n_kept", "n_limit", "n_error", "n_edge", "n_rounds", "n_hist_rounds"):
                    tot[k] += int(getattr(i, k))
                tot["arena_peak_bytes"] = max(tot["arena_peak_bytes"], int(i.arena_bytes))
                for k in ("ms_upload", "ms_jobs", "ms_score", "ms_hist", "ms_back", "ms_host"):
                    tot[k] += float(getattr(i, k))
                tot["ms_call"] += float(i.ms_wall)
            tot["wall_ms"] = (time.perf_counter() - t) * 1e3
            runs.append(tot)
        best = min(runs, key=lambda r: r["wall_ms"])
        out = dict(workload=w, n_sc=SIZES[w], contigs=len(work), n_variants=int(sum(len(h["pos"]) for h, _, _ in work)), best=best,
                   gpu_clusters_per_s=best["n_clusters"] / (best["wall_ms"] / 1e3), all_runs=runs)
        if args.cpu_clusters > 0:
            h, cl, seq = max(work, key=lambda x: x[1].n)
            k = min(args.cpu_clusters, cl.n)
            tmp = tempfile.mkdtemp(prefix="realign_bench_")
            path = os.path.join(tmp, "w.npz")
            np.savez(path, seq=np.asarray(seq, np.uint8), var_beg=cl.var_beg, **{c: h[c] for c in COLS})
            cuts = np.linspace(0, k, args.cpu_procs + 1).astype(int)
            parts = [(path, int(cuts[p]), int(cuts[p + 1])) for p in range(args.cpu_procs)]
            t = time.perf_counter()
            with mp.get_context("spawn").Pool(args.cpu_procs) as pool:
                got = pool.map(_cpu_part, parts)
            wall = time.perf_counter() - t
            out["cpu_model"] = dict(clusters=k, procs=args.cpu_procs, wall_s=wall, max_part_s=max(g[1] for g in got),
                                    clusters_per_s=k / max(max(g[1] for g in got), 1e-9))
        print(json.dumps(out), flush=True)
        lines.append(out)
        del syn, v, work
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
