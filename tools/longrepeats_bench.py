"""Times vpr_longrepeat_intervals (--stratify-long-repeats, include/vcfdist_longrepeats.h) with the default set on the synthetic
50 Mb contig of tools/repeats_bench.py (copies of 40 to 5000 bases planted every 50 kb).  Device ms of the four phases -- base
level, doubling levels, last levels with the mark, intervals -- for the set and per entry (HIP events, the best of --reps calls),
the pairs every level sorted, and in the same run rep_k32 alone through vpr_repeat_intervals and the bare sort of as many random
keys as the base level sorts (vpr_repeat_sort_floor).  The claim to check: the upper levels, which sort candidates only, cost less
than the base level.  Beside it the model (tests/longrepeats_model.py) on the first 2 Mb of the contig, whose intervals the GPU's
on that slice must equal -- that equality is the gate, there is no threshold on time.  One JSON line; --out also writes a file.

    python tools/longrepeats_bench.py [--bases 50000000] [--model-bases 2000000] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = ("ms_base", "ms_levels", "ms_last", "ms_intervals")


def best_call(pr, contigs, specs, reps):
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        pr.longrepeat_intervals(contigs, specs)
        wall = time.perf_counter() - t
        ms = pr.longrepeat_timing()
        runs.append(dict(zip(PHASES, ms), ms_total=sum(ms), wall_ms=wall * 1e3))
    return min(runs, key=lambda r: r["ms_total"]), runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--model-bases", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import longrepeats_model as LM
    import repeats_bench as RB
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api
    names, specs = api.longrepeats_default()
    seq = RB.make_contig(args.bases, args.seed)
    pr = api.PrecisionRecall()
    pr.longrepeat_intervals([seq], specs)           # warm-up: code objects, workspaces
    best, runs = best_call(pr, [seq], specs, args.reps)
    n_valid, n_rep, n_last, n_level = pr.longrepeat_stats(levels=True)
    rows = pr.download_longrepeat_intervals()
    n_iv = {n: int(len(r[0][0])) for n, r in zip(names, rows)}
    assert all(n_iv.values()), n_iv
    entries = {}
    for n, sp, nv, nr, nl in zip(names, specs, n_valid, n_rep, n_last):
        b, _ = best_call(pr, [seq], [sp], args.reps)
        lv = pr.longrepeat_stats(levels=True)[3]
        entries[n] = dict(k=sp.k, valid_starts=int(nv), repeated_starts=int(nr), last_level_candidates=int(nl),
                          level_pairs=dict(base=int(lv[0]), level64=int(lv[1]), level128=int(lv[2])), **b)
    # rep_k32 alone through vpr_repeat_intervals, and the bare sort at the base level's size
    k32 = []
    for _ in range(args.reps + 1):
        pr.repeat_intervals([seq], [A.rep_kmer(32)])
        ms = pr.repeat_timing()
        k32.append(dict(zip(RB.PASSES, ms), ms_total=sum(ms)))
    k32 = min(k32[1:], key=lambda r: r["ms_total"])
    floor = min(pr.repeat_sort_floor(int(n_level[0]), 32, seed=s + 1) for s in range(args.reps))
    upper = best["ms_levels"] + best["ms_last"]
    out = dict(bases=args.bases, strata=len(specs), intervals=n_iv, best=best, all_runs=runs, entries=entries,
               level_pairs=dict(base=int(n_level[0]), level64=int(n_level[1]), level128=int(n_level[2]),
                                last={n: int(x) for n, x in zip(names, n_last)}),
               rep_k32_alone=k32, sort_floor_ms_base=floor, ms_over_rep_k32=best["ms_total"] / k32["ms_total"],
               base_share=best["ms_base"] / best["ms_total"], upper_levels_ms=upper, upper_below_base=bool(upper < best["ms_base"]),
               bases_per_s=args.bases / (best["ms_total"] / 1e3))
    if args.model_bases > 0:
        k = min(args.model_bases, args.bases)
        part = np.ascontiguousarray(seq[:k])
        t = time.perf_counter()
        want, want_valid, want_rep = LM.all_intervals([part], specs)
        model_s = time.perf_counter() - t
        pr.longrepeat_intervals([part], specs)
        bad = LM.same(pr.download_longrepeat_intervals(), want)
        got_valid, got_rep = pr.longrepeat_stats()
        assert not bad and np.array_equal(got_valid, want_valid) and np.array_equal(got_rep, want_rep), (bad, got_valid, want_valid, got_rep, want_rep)
        out["model"] = dict(bases=k, wall_s=model_s, bases_per_s=k / model_s, gpu_ms_same_slice=sum(pr.longrepeat_timing()),
                            intervals=[int(len(r[0][0])) for r in want], equal=True)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
