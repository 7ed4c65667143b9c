"""Times vpr_distance (-d, include/vcfdist_distance.h) on the synthetic workloads of bench.py: wgs_synth (1 M superclusters),
joint_synth (100 k) and sv_synth (200).  Per workload: kernel time of each pass (job listing, pass 1 score, pass 2 history, backtracks),
wall time of the call, jobs/s, rounds and the peak arena bytes; beside it the CPU model (tests/distance_model.cpp) on 16 processes over
a slice of the same superclusters (--cpu-sc), as jobs/s.  One JSON line per workload; --out also writes them to a file.

    python tools/distance_bench.py [--workloads wgs_synth,joint_synth,sv_synth] [--reps 3] [--cpu-sc 20000] [--out FILE]"""
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

SIZES = {"wgs_synth": 1_000_000, "joint_synth": 100_000, "sv_synth": 200}


FIELDS = ("ctg_off", "ctg_seq", "sc_ctg", "sc_beg", "sc_end")
SLOT_FIELDS = ("var_off", "var_pos", "var_type", "var_qual", "var_ref_len", "var_alt_len", "var_alt_off", "allele_pool")


def _cpu_part(arg):
    """a worker (spawned: it never opens the GPU) runs the model over superclusters [lo, hi) of the saved workload"""
    path, lo, hi = arg
    import types
    import distance_helpers as DH
    z = np.load(path)
    v = types.SimpleNamespace(**{f: z[f] for f in FIELDS})
    v.n_sc = len(v.sc_beg)
    for f in SLOT_FIELDS:
        setattr(v, f, [z[f"{f}{s}"] for s in range(4)])
    sc_phase, skip = z["sc_phase"], z["skip"]
    sk = skip.copy()
    sk[:lo] = 1
    sk[hi:] = 1
    t = time.perf_counter()
    jobs, _ = DH.run(v, sc_phase, sk)
    return len(jobs), time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="wgs_synth,joint_synth,sv_synth")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cpu-sc", type=int, default=20000, help="superclusters the CPU model runs on (0: none)")
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    import distance_helpers as DH
    from vcfdist_amd import api
    DH.model()                  # compiled once, before the workers fork
    lines = []
    for w in args.workloads.split(","):
        n_sc = SIZES[w]
        syn = bench.make_workload(api, n_sc, args.seed, w)
        batch = syn.batch(copy=False)
        v = syn.variants()
        pr = api.PrecisionRecall()
        res = pr.run(batch)
        runs = []
        for _ in range(args.reps):
            t = time.perf_counter()
            d = pr.distance(v)
            wall = time.perf_counter() - t
            i = d["info"]
            runs.append(dict(wall_ms=wall * 1e3, ms_upload=i.ms_upload, ms_jobs=i.ms_jobs, ms_score=i.ms_score, ms_hist=i.ms_hist,
                             ms_back=i.ms_back, ms_call=i.ms_wall))
        best = min(runs, key=lambda r: r["wall_ms"])
        out = dict(workload=w, n_sc=n_sc, n_jobs=int(i.n_jobs), n_edits=int(i.n_edits), n_limit=int(i.n_limit), n_error=int(i.n_error),
                   n_rounds=int(i.n_rounds), n_hist_rounds=int(i.n_hist_rounds), arena_peak_bytes=int(i.arena_bytes),
                   input_bytes=int(i.input_bytes), history_cells=int(i.history_cells), best=best,
                   gpu_jobs_per_s=int(i.n_jobs) / (best["wall_ms"] / 1e3), all_runs=runs)
        if args.cpu_sc > 0:
            k = min(args.cpu_sc, n_sc)
            skip = np.zeros(n_sc, np.uint8)
            skip[np.nonzero(res.aln_status & np.uint32(32 | 64 | 128))[0] // 4] = 1
            cuts = np.linspace(0, k, args.cpu_procs + 1).astype(int)
            tmp = tempfile.mkdtemp(prefix="distance_bench_")
            path = os.path.join(tmp, "w.npz")
            arrs = {f: getattr(v, f) for f in FIELDS}
            arrs.update({f"{f}{s}": getattr(v, f)[s] for f in SLOT_FIELDS for s in range(4)})
            np.savez(path, sc_phase=np.asarray(res.sc_phase, np.int32), skip=skip, **arrs)
            parts = [(path, int(cuts[p]), int(cuts[p + 1])) for p in range(args.cpu_procs)]
            t = time.perf_counter()
            with mp.get_context("spawn").Pool(args.cpu_procs) as pool:
                got = pool.map(_cpu_part, parts)
            wall = time.perf_counter() - t
            nj = sum(g[0] for g in got)
            out["cpu_model"] = dict(superclusters=k, procs=args.cpu_procs, jobs=nj, wall_s=wall, max_part_s=max(g[1] for g in got),
                                    jobs_per_s=nj / max(max(g[1] for g in got), 1e-9))
        print(json.dumps(out), flush=True)
        lines.append(out)
        del pr, res, batch, syn
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
