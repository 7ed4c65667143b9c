"""Times vpr_nearrepeat_intervals (--stratify-near-repeats, include/vcfdist_nearrepeats.h) on the 50 Mb contig of tools/repeats_bench.py
with mutated copies added: words of 40 to 5000 bases, each with substitutions at a rate of 1 to 3 per 32 bases, forward and
reverse-complemented.  Per entry -- 32:1, 32:2, 24:1, each alone -- the device ms of the four passes (pack, sort, probe, intervals;
HIP events, the best of --reps calls), the compares, the longest run of equal block keys, the valid and the near-repeated starts;
beside them, in the same run, rep_k32 alone through vpr_repeat_intervals, and every entry's ratio to it.  The gate is equality with
the numpy model (tests/nearrepeats_model.py) on the first --model-bases of the same contig; there is no threshold on time.  One JSON
line; --out also writes it to a file.

    python tools/nearrepeats_bench.py [--bases 50000000] [--model-bases 1000000] [--reps 5] [--out FILE]"""
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

PASSES = ("ms_pack", "ms_sort", "ms_probe", "ms_intervals")
REP_PASSES = ("ms_pack", "ms_sort", "ms_mark", "ms_intervals")
ENTRIES = ((32, 1), (32, 2), (24, 1))


def make_contig(n, seed):
    """repeats_bench's contig with a mutated copy every 50 kb, 10 kb behind its exact one: a word of 40 to 5000 bases taken from
    25 kb further on, 1 to 3 substitutions per 32 bases, every other one reverse-complemented"""
    import repeats_bench as RB
    import repeats_cases as RC
    seq = RB.make_contig(n, seed)
    rng = np.random.RandomState(seed + 11)
    other = np.frombuffer(b"CGTA", np.uint8)                     # (another base for A, C, G, T; anything else becomes A)
    for i, pos in enumerate(range(40_000, n - 40_000, 50_000)):
        m = int(rng.choice([40, 100, 400, 1500, 5000]))
        w = np.frombuffer(bytes(seq[pos + 25_000:pos + 25_000 + m]), np.uint8).copy()
        hit = rng.random_sample(m) < int(rng.randint(1, 4)) / 32.0
        code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), w[hit]) & 3
        w[hit] = other[code]
        w = bytes(w)
        seq[pos:pos + m] = np.frombuffer(RC.revcomp(w) if i % 2 else w, np.uint8)
    return seq


def best_call(call, timing, passes, reps):
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        wall = time.perf_counter() - t
        ms = timing()
        runs.append(dict(zip(passes, ms), ms_total=sum(ms), wall_ms=wall * 1e3))
    return min(runs, key=lambda r: r["ms_total"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--model-bases", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import nearrepeats_model as NM
    from vcfdist_amd import _abi as A, api
    seq = make_contig(args.bases, args.seed)
    pr = api.PrecisionRecall()
    rep = [A.rep_kmer(32)]
    pr.repeat_intervals([seq], rep)                 # warm-up: code objects, workspaces
    exact = best_call(lambda: pr.repeat_intervals([seq], rep), pr.repeat_timing, REP_PASSES, args.reps)
    rep_valid, rep_rep = pr.repeat_stats()
    exact.update(valid_starts=int(rep_valid[0]), repeated_starts=int(rep_rep[0]))
    entries = {}
    for k, m in ENTRIES:
        spec = [A.near_kmer(k, m)]
        pr.nearrepeat_intervals([seq], spec)        # warm-up
        b = best_call(lambda: pr.nearrepeat_intervals([seq], spec), pr.nearrepeat_timing, PASSES, args.reps)
        n_valid, n_near, compares, max_run = pr.nearrepeat_stats(cost=True)
        n_iv = int(len(pr.download_nearrepeat_intervals()[0][0][0]))
        assert n_iv > 0
        entries[api.nearrepeat_name(spec[0])] = dict(k=k, m=m, **b, valid_starts=int(n_valid[0]), near_repeated_starts=int(n_near[0]),
                                                     compares=int(compares[0]), longest_run=int(max_run[0]), intervals=n_iv,
                                                     compares_per_valid_start=float(compares[0]) / max(int(n_valid[0]), 1),
                                                     over_rep_k32=b["ms_total"] / exact["ms_total"])
    # the gate: the model on a slice, as a genome of its own
    head = seq[:args.model_bases]
    spec = [A.near_kmer(32, 1), A.near_kmer(24, 1)]
    t = time.perf_counter()
    want = NM.all_intervals([bytes(head)], spec)
    model_s = time.perf_counter() - t
    pr.nearrepeat_intervals([head], spec)
    got_valid, got_near = pr.nearrepeat_stats()
    equal = not NM.same(pr.download_nearrepeat_intervals(), want[0]) and np.array_equal(got_valid, want[1]) and np.array_equal(got_near, want[2])
    out = dict(bases=args.bases, reps=args.reps, rep_k32=exact, entries=entries, model_bases=args.model_bases, model_seconds=model_s,
               model_near_repeated_starts=[int(x) for x in want[2]], equals_model=bool(equal),
               note="one synthetic contig; what a real genome's longest runs cost is not measured")
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        sys.exit("the GPU's intervals differ from the model's on the slice")


if __name__ == "__main__":
    main()
