"""Times vpr_repeat_intervals (--stratify-repeats, include/vcfdist_repeats.h) with the default set on one synthetic contig of 50 Mb:
the contig of tools/context_bench.py with copies planted (forward and reverse-complemented, 40 to 5000 bases), so that no
stratum is empty.  Device ms of the four passes -- pack, sort, mark, intervals -- per entry and in total (HIP events, the best of
--reps calls), starts per second, and as the floor a bare vplan_sort_pairs_u64 of as many random 64-bit keys (the sort moves 24
bytes per key and radix pass; every other pass moves less than one sort pass).  Beside it the numpy model (tests/repeats_model.py)
on the first 5 Mb of the same contig, whose intervals the GPU's on that slice must equal -- that equality is the gate, there is
no threshold on time -- and the figure of profiles/context_bench.json for the same contig, for scale.  One JSON line; --out also
writes it to a file.

    python tools/repeats_bench.py [--bases 50000000] [--model-bases 5000000] [--reps 5] [--out FILE]"""
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

PASSES = ("ms_pack", "ms_sort", "ms_mark", "ms_intervals")


def make_contig(n, seed):
    """context_bench's contig with a copy planted every 50 kb: a word of 40 to 5000 bases taken from 20 kb further on, every other
    one reverse-complemented (the first 5 Mb hold a hundred of them, so the model's slice is not empty either)"""
    import context_bench as CB
    import repeats_cases as RC
    seq = CB.make_contig(n, seed)
    rng = np.random.RandomState(seed + 7)
    for i, pos in enumerate(range(30_000, n - 40_000, 50_000)):
        m = int(rng.choice([40, 100, 400, 1500, 5000]))
        w = bytes(seq[pos + 20_000:pos + 20_000 + m])
        seq[pos:pos + m] = np.frombuffer(RC.revcomp(w) if i % 2 else w, np.uint8)
    return seq


def best_call(pr, contigs, specs, reps):
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        pr.repeat_intervals(contigs, specs)
        wall = time.perf_counter() - t
        ms = pr.repeat_timing()
        runs.append(dict(zip(PASSES, ms), ms_total=sum(ms), wall_ms=wall * 1e3))
    return min(runs, key=lambda r: r["ms_total"]), runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--model-bases", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import repeats_model as RM
    from vcfdist_amd import api
    names, specs = api.repeats_default()
    seq = make_contig(args.bases, args.seed)
    pr = api.PrecisionRecall()
    pr.repeat_intervals([seq], specs)               # warm-up: code objects, workspaces
    best, runs = best_call(pr, [seq], specs, args.reps)
    n_valid, n_rep = pr.repeat_stats()
    rows = pr.download_repeat_intervals()
    n_iv = {n: int(len(r[0][0])) for n, r in zip(names, rows)}
    assert all(n_iv.values()), n_iv
    entries = {}
    for n, sp, nv, nr in zip(names, specs, n_valid, n_rep):
        b, _ = best_call(pr, [seq], [sp], args.reps)
        floor = min(pr.repeat_sort_floor(int(nv), sp.k, seed=s + 1) for s in range(args.reps))
        entries[n] = dict(k=sp.k, valid_starts=int(nv), repeated_starts=int(nr), **b, sort_floor_ms=floor, sort_share=b["ms_sort"] / b["ms_total"],
                          sort_over_floor=b["ms_sort"] / floor, key_bits=2 * sp.k)
    starts = int(n_valid.sum())
    out = dict(bases=args.bases, strata=len(specs), intervals=n_iv, best=best, all_runs=runs, entries=entries, valid_starts=starts,
               starts_per_s=starts / (best["ms_total"] / 1e3), bases_per_s=args.bases / (best["ms_total"] / 1e3),
               sort_share=best["ms_sort"] / best["ms_total"], sort_floor_ms_total=sum(e["sort_floor_ms"] for e in entries.values()))
    if args.model_bases > 0:
        k = min(args.model_bases, args.bases)
        part = np.ascontiguousarray(seq[:k])
        t = time.perf_counter()
        want, want_valid, want_rep = RM.all_intervals([part], specs)
        model_s = time.perf_counter() - t
        pr.repeat_intervals([part], specs)
        bad = RM.same(pr.download_repeat_intervals(), want)
        got_valid, got_rep = pr.repeat_stats()
        assert not bad and np.array_equal(got_valid, want_valid) and np.array_equal(got_rep, want_rep), (bad, got_valid, want_valid, got_rep, want_rep)
        out["numpy_model"] = dict(bases=k, wall_s=model_s, bases_per_s=k / model_s, gpu_ms_same_slice=sum(pr.repeat_timing()),
                                  intervals=[int(len(r[0][0])) for r in want], equal=True)
    ctx = os.path.join(ROOT, "profiles", "context_bench.json")
    if os.path.exists(ctx):
        c = json.load(open(ctx))
        out["context_bench_for_scale"] = dict(bases=c.get("bases"), strata=c.get("strata"), ms_intervals=c.get("best", {}).get("ms_intervals"),
                                              bases_per_s=c.get("bases_per_s"))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
