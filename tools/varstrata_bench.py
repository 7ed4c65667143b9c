"""Times vpr_varstrata_masks (--stratify-variants, include/vcfdist_varstrata.h) with the default set on a wgs_synth-shaped batch of
about a million hap-variants: the device time of the k_varstrata_mask launches (HIP events on the handle's stream, the best of
--reps calls).  Beside it, in the same run and on the same variants, the yardstick already in the tree: the device time of
k_strata_mask (vpr_strata_timing) for as many BED strata of --intervals random intervals each; and the brute-force model
(tests/varstrata_model.py) on the first --model-sc superclusters, whose bits the GPU's on that slice must equal.  No threshold is
set.  One JSON line; --out also writes it to a file.

    python tools/varstrata_bench.py [--n-sc 330000] [--intervals 100000] [--model-sc 1500] [--reps 5] [--out profiles/varstrata_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def first_superclusters(A, v, n):
    """the first n superclusters of v as an A.Variants of their own"""
    off = [np.ascontiguousarray(v.var_off[h][:n + 1]) for h in range(4)]
    cut = lambda cols: [np.ascontiguousarray(cols[h][:int(off[h][-1])]) for h in range(4)]
    return A.Variants(v.ctg_off, v.ctg_seq, v.sc_ctg[:n], v.sc_beg[:n], v.sc_end[:n], off, cut(v.var_pos), cut(v.var_type), cut(v.var_qual),
                      cut(v.var_ref_off), cut(v.var_ref_len), cut(v.var_alt_off), cut(v.var_alt_len), v.allele_pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sc", type=int, default=330_000)
    ap.add_argument("--intervals", type=int, default=100_000)
    ap.add_argument("--model-sc", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    import varstrata_model as VM
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api, io as IO
    names, specs = api.varstrata_default()
    v = bench.make_workload(api, args.n_sc, args.seed, "wgs_synth").variants()
    n_var = [v.n_vars(h) for h in range(4)]
    length = int(v.ctg_off[1])
    pr = api.PrecisionRecall()
    runs = []
    for _ in range(args.reps + 1):        # (the first repetition warms up: code objects, allocations)
        t = time.perf_counter()
        pr.varstrata_masks(v, specs)
        runs.append(dict(k_varstrata_mask_ms=pr.varstrata_timing(), wall_ms=(time.perf_counter() - t) * 1e3))
    runs = runs[1:]
    words = pr.download_strata_masks()
    members = {n: int(sum(int(((w[0] >> np.uint64(k)) & np.uint64(1)).sum()) for w in words)) for k, n in enumerate(names)}
    # the yardstick: the BED membership kernel for the same number of strata on the same variants
    rng = np.random.RandomState(args.seed)
    tmp = tempfile.mkdtemp(prefix="varstrata_bench_")
    beds = []
    for k in range(len(specs)):
        cuts = np.sort(rng.choice(length - 1, size=2 * args.intervals, replace=False)) + 1
        p = os.path.join(tmp, f"s{k}.bed")
        np.savetxt(p, np.stack([cuts[0::2], cuts[1::2]], 1), fmt="c0\t%d\t%d")
        beds.append(IO.Bed(p))
    strata = IO.contig_strata(beds, ["c0"])
    bed_runs = []
    for _ in range(args.reps + 1):
        pr.strata_masks(v, strata)
        bed_runs.append(pr.strata_timing()[0])
    bed_runs = bed_runs[1:]
    best, bed_best = min(r["k_varstrata_mask_ms"] for r in runs), min(bed_runs)
    out = dict(workload="wgs_synth", n_sc=args.n_sc, hap_variants=int(sum(n_var)), strata=len(specs), members=members,
               k_varstrata_mask_ms=best, hap_variants_per_s=sum(n_var) / (best / 1e3), all_runs=runs,
               bed_yardstick=dict(strata=len(specs), intervals_per_stratum=args.intervals, k_strata_mask_ms=bed_best, all_runs=bed_runs),
               varstrata_over_bed=best / max(bed_best, 1e-9))
    if args.model_sc > 0:
        part = first_superclusters(A, v, min(args.model_sc, v.n_sc))
        t = time.perf_counter()
        bits = VM.members(part, specs)
        model_s = time.perf_counter() - t
        pr.varstrata_masks(part, specs)
        got = pr.download_strata_masks()
        same = all(np.array_equal(got[h], VM.words_of(bits[h])) for h in range(4))
        n_part = int(sum(part.n_vars(h) for h in range(4)))
        out["model"] = dict(superclusters=part.n_sc, hap_variants=n_part, wall_s=model_s, hap_variants_per_s=n_part / model_s,
                            gpu_ms_same_slice=pr.varstrata_timing(), equal=bool(same))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if args.model_sc > 0 and not out["model"]["equal"]:
        raise SystemExit("the device's membership words differ from the model's")


if __name__ == "__main__":
    main()
