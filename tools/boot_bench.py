"""Times the bootstrap replicates of the counters (include/vcfdist_bootstrap.h) on one MI355X: the device time of the
k_pr_boot launches (HIP events on the handle's stream, vpr_boot_info) for 64 and 1 000 replicates on wgs_synth and joint_synth
batches, and beside it, in the same run and on the same executed batch:
  - the plain vpr_pr_counts (host wall time of the call with resident classes: an upper bound of k_pr_hist's device time),
  - one execute step (kernel time of vpr_execute, vpr_get_timing),
  - the comparator: vpr_pr_counts_strata with as many strata as replicates, each covering every variant (all membership bits
    set): the lane-per-variant shape doing n_var x n_rep LDS increments (vpr_strata_timing).
The replicates at weight 1 (all keys equal, a replicate whose weight is 1) are compared with the comparator's counts.  One
JSON line; --out also writes it to a file.

    python tools/boot_bench.py [--workloads wgs_synth:1000000,joint_synth:100000] [--reps 5] [--out profiles/boot_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs))


def one_workload(api, S, A, bench, name, n_sc, seed, replicates, reps):
    syn = bench.make_workload(api, n_sc, seed, name)
    pr = api.PrecisionRecall()
    res = pr.run(syn.batch(copy=False))
    execute_ms = float(pr.timing().ms_total)
    cls = syn.var_class()
    pb, _, _ = S.phase(res.sc_phase, np.ones(n_sc, np.int32))
    plain = S.pr_counts(pr, cls, pb)
    n_var = [int(len(c)) for c in cls]
    keys = A.boot_keys(0, np.arange(n_sc))
    wall = []
    for _ in range(reps + 1):
        t = time.perf_counter()
        S.pr_counts(pr, None, pb)
        wall.append((time.perf_counter() - t) * 1e3)
    out = dict(workload=name, n_sc=n_sc, hap_variants=sum(n_var), execute_kernels_ms=execute_ms, pr_counts_wall_ms=spread(wall[1:]), replicates={})
    for n_rep in replicates:
        # the comparator: n_rep strata that each hold every variant
        nw = (n_rep + 63) // 64
        word = np.full(nw, np.uint64(2 ** 64 - 1), np.uint64)
        if n_rep % 64:
            word[-1] = np.uint64((1 << (n_rep % 64)) - 1)
        pr.upload_strata_masks(n_rep, [np.repeat(word[:, None], n, axis=1) for n in n_var])
        boot, comp, grid = [], [], None
        for _ in range(reps + 1):         # the two alternate; the first repetition warms up (code objects, allocations)
            got = pr.pr_counts_boot(None, pb, keys, n_rep, 1)
            grid, ms = pr.boot_info()
            boot.append(ms)
            strat = S.pr_counts_strata(pr, None, pb)
            comp.append(pr.strata_timing()[1])
        nonzero = float((np.asarray([int(g[:, 3, :, 0].sum()) for g in got[:8]]) > 0).mean())
        # weight 1 for every supercluster reproduces a stratum that covers everything
        same = pr.pr_counts_boot(None, pb, np.full(n_sc, 1, np.uint64), 1, 1)[0]
        ok = bool(np.array_equal(same, strat[0]) and np.array_equal(strat[0], plain) and np.array_equal(strat[-1], plain))
        out["replicates"][str(n_rep)] = dict(k_pr_boot_ms=spread(boot[1:]), grid=list(grid), comparator_k_pr_hist_strata_ms=spread(comp[1:]),
                                             boot_over_comparator=float(np.median(boot[1:]) / np.median(comp[1:])),
                                             weight_one_equals_comparator=ok, first_replicates_nonzero=nonzero, all_boot_ms=boot[1:],
                                             all_comparator_ms=comp[1:])
        if not ok:
            raise SystemExit(f"{name}: the replicates at weight 1 differ from the stratified counters")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="wgs_synth:1000000,joint_synth:100000")
    ap.add_argument("--replicates", default="64,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api, summary as S
    # (the weight of key 1, replicate 0, seed 1 is 1: the weight-one comparison below relies on it)
    runs = []
    for w in args.workloads.split(","):
        name, n_sc = w.split(":")
        runs.append(one_workload(api, S, A, bench, name, int(n_sc), args.seed, [int(x) for x in args.replicates.split(",")], args.reps))
    out = dict(waves=os.environ.get("VPR_BOOT_WAVES", "default"), wg_target=os.environ.get("VPR_BOOT_WG_TARGET", "default"), runs=runs)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
