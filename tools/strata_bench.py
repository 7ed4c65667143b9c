"""Times the region-stratified counters (include/vcfdist_strata.h) on a wgs_synth-shaped batch of about a million hap-variants
against 64 strata of 100 000 random intervals each: the device time of k_strata_mask and of the k_pr_hist_strata launches (HIP
events on the handle's stream, vpr_strata_timing), beside them the unstratified vpr_pr_counts of the same batch (host wall time
of the call with resident classes: launch, synchronise and a 9 KB copy around k_pr_hist -- an upper bound of its device time), and
the wall time of the same memberships through the host's vio_bed_contains loop on one thread (vio_bed_contains_many), in the same
run.  The words of the two are compared.  One JSON line; --out also writes it to a file.

    python tools/strata_bench.py [--n-sc 330000] [--strata 64] [--intervals 100000] [--reps 5] [--out profiles/strata_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sc", type=int, default=330_000)
    ap.add_argument("--strata", type=int, default=64)
    ap.add_argument("--intervals", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    from vcfdist_amd import api, io as IO, summary as S
    syn = bench.make_workload(api, args.n_sc, args.seed, "wgs_synth")
    v = syn.variants()
    length = int(v.ctg_off[1])
    n_var = [v.n_vars(h) for h in range(4)]
    rng = np.random.RandomState(args.seed)
    tmp = tempfile.mkdtemp(prefix="strata_bench_")
    beds = []
    for k in range(args.strata):
        cuts = np.sort(rng.choice(length - 1, size=2 * args.intervals, replace=False)) + 1
        p = os.path.join(tmp, f"s{k}.bed")
        np.savetxt(p, np.stack([cuts[0::2], cuts[1::2]], 1), fmt="c0\t%d\t%d")
        beds.append(IO.Bed(p))
    strata = IO.contig_strata(beds, ["c0"])
    pr = api.PrecisionRecall()
    res = pr.run(syn.batch(copy=False))
    cls = syn.var_class()
    pb, _, _ = S.phase(res.sc_phase, np.ones(v.n_sc, np.int32))
    S.pr_counts(pr, cls, pb)
    runs = []
    for _ in range(args.reps + 1):        # (the first repetition warms up: code objects, allocations)
        pr.strata_masks(v, strata)
        counts = S.pr_counts_strata(pr, None, pb)
        ms_mask, ms_hist = pr.strata_timing()
        t = time.perf_counter()
        plain = S.pr_counts(pr, None, pb)
        runs.append(dict(k_strata_mask_ms=ms_mask, k_pr_hist_strata_ms=ms_hist, pr_counts_wall_ms=(time.perf_counter() - t) * 1e3))
    runs = runs[1:]
    words = pr.download_strata_masks()
    t = time.perf_counter()
    loc = [np.stack([b.contains_many("c0", v.var_pos[h], v.var_ref_len[h], v.var_type[h]) for b in beds]) for h in range(4)]
    host_s = time.perf_counter() - t
    same = True
    for h in range(4):
        w = np.zeros_like(words[h])
        for k in range(args.strata):
            w[k >> 6] |= (loc[h][k] == 1).astype(np.uint64) << np.uint64(k & 63)
        same = same and bool(np.array_equal(w, words[h]))
    med = {f: float(np.median([r[f] for r in runs])) for f in runs[0]}
    device_ms = med["k_strata_mask_ms"] + med["k_pr_hist_strata_ms"]
    out = dict(workload="wgs_synth", n_sc=args.n_sc, hap_variants=int(sum(n_var)), strata=args.strata, intervals_per_stratum=args.intervals,
               lookups=int(sum(n_var)) * args.strata, median=med, device_ms=device_ms, host_loop_ms=host_s * 1e3,
               host_ns_per_lookup=host_s * 1e9 / (sum(n_var) * args.strata), host_over_device=host_s * 1e3 / max(device_ms, 1e-9),
               words_equal_host=same, members=int(sum(int((l == 1).sum()) for l in loc)),
               counted=int(plain[:, 3, :, 0].sum()), counted_in_strata=int(counts[:, :, 3, :, 0].sum()), all_runs=runs)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not same:
        raise SystemExit("the device's membership words differ from the host loop's")
    if device_ms >= host_s * 1e3:
        raise SystemExit("masks plus stratified histogram take no less device time than the host loop takes wall time")


if __name__ == "__main__":
    main()
