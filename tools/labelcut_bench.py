"""Times the label counts cut by stratum and resampled (--cut-classes, include/vcfdist_labelcut.h) on the evaluated wgs_synth-shaped
batch of tools/errclass_bench.py (about a million hap-variants) under the fourteen default variant strata: the device time of the
k_label_hist_strata launches of both label passes beside k_pr_hist_strata on the same membership words, and of the k_label_boot
launches at --n-rep replicates of both passes beside k_pr_boot -- HIP events on the handle's stream, the best of --reps calls, all
in one run.  The sums of the labels are held to the counters' columns.  No threshold is set.  One JSON line; --out also writes it
to a file.

    python tools/labelcut_bench.py [--n-sc 330000] [--n-rep 1000] [--reps 5] [--out profiles/labelcut_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sc", type=int, default=330_000)
    ap.add_argument("--n-rep", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api, summary as S
    syn = bench.make_workload(api, args.n_sc, args.seed, "wgs_synth")
    v = syn.variants()
    n_var = [v.n_vars(h) for h in range(4)]
    cls = syn.var_class()
    pr = api.PrecisionRecall()
    res = pr.run(syn.batch(copy=False))
    pb, _, _ = S.phase(res.sc_phase, np.ones(v.n_sc, np.int32))
    S.pr_counts(pr, cls, pb)
    names, specs = api.varstrata_default()
    pr.varstrata_masks(v, specs)
    keys = A.boot_keys(0, np.arange(v.n_sc))
    point = dict(errclass=pr.errclass(v, None, pb), matchkind=pr.matchkind(v, None, pb))
    sums = dict(errclass=(A.ERRTYPE_FP, A.ERRTYPE_FN), matchkind=(A.ERRTYPE_TP, A.ERRTYPE_TP))
    n_all = sum(n_var)
    labelled = {p: int(c[0, 3, :, 0].sum() + c[1, 3].sum(0).max()) for p, c in point.items()}      # query at threshold 0, truth at its fullest
    strata = dict(k_pr_hist_strata=[], errclass=[], matchkind=[])
    boot = dict(k_pr_boot=[], errclass=[], matchkind=[])
    ok = True
    for _ in range(args.reps + 1):        # (the first repetition warms up: code objects, allocations)
        strat = S.pr_counts_strata(pr, None, pb)
        strata["k_pr_hist_strata"].append(pr.strata_timing()[1])
        reps = pr.pr_counts_boot(None, pb, keys, args.n_rep, args.seed)
        boot["k_pr_boot"].append(pr.boot_info()[1])
        for p in ("errclass", "matchkind"):
            a = getattr(pr, p + "_strata")()
            strata[p].append(getattr(pr, p + "_cut_timing")()[0])
            b = getattr(pr, p + "_boot")(keys, args.n_rep, args.seed)
            boot[p].append(getattr(pr, p + "_cut_timing")()[1])
            for cs in range(2):
                ok = ok and np.array_equal(a[:, cs].sum(2), strat[:, cs, :, sums[p][cs]]) and np.array_equal(b[:, cs].sum(2), reps[:, cs, :, sums[p][cs]])
    best = lambda d: {k: min(x[1:]) for k, x in d.items()}
    bs, bb = best(strata), best(boot)
    out = dict(workload="wgs_synth", n_sc=args.n_sc, hap_variants=int(n_all), n_strata=len(names), n_rep=args.n_rep, thresholds=61,
               labelled=labelled, labelled_share={p: n / n_all for p, n in labelled.items()}, sums_hold=bool(ok),
               strata_ms=dict(k_pr_hist_strata=bs["k_pr_hist_strata"], k_label_hist_strata_errclass=bs["errclass"],
                              k_label_hist_strata_matchkind=bs["matchkind"]),
               strata_over_counters=dict(errclass=bs["errclass"] / max(bs["k_pr_hist_strata"], 1e-9), matchkind=bs["matchkind"] / max(bs["k_pr_hist_strata"], 1e-9)),
               strata_shape={p: getattr(pr, p + "_cut_info")() for p in ("errclass", "matchkind")},
               boot_ms=dict(k_pr_boot=bb["k_pr_boot"], k_label_boot_errclass=bb["errclass"], k_label_boot_matchkind=bb["matchkind"]),
               boot_over_counters=dict(errclass=bb["errclass"] / max(bb["k_pr_boot"], 1e-9), matchkind=bb["matchkind"] / max(bb["k_pr_boot"], 1e-9)),
               boot_grid_counters=list(pr.boot_info()[0]),
               all_runs=dict(strata={k: x[1:] for k, x in strata.items()}, boot={k: x[1:] for k, x in boot.items()}))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not ok:
        raise SystemExit("the labels do not sum to the counters' columns")


if __name__ == "__main__":
    main()
