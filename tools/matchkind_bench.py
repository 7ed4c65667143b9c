"""Times vpr_matchkind (--classify-matches, include/vcfdist_matchkind.h) on the batch of tools/errclass_bench.py, an evaluated
wgs_synth-shaped batch of about a million hap-variants: the device time of the k_matchkind launches (HIP events on the handle's
stream, the best of --reps calls).  Beside it, in the same run and on the same batch, the two kernels it stands beside: the
k_errclass launches of vpr_errclass and the k_varstrata_mask launches of the default variant strata.  It records the number of TP per
kind, the largest supercluster's variant count (the length of the longest member scan), and whether the GPU's kind bytes equal the
brute-force model's (tests/matchkind_model.py) on the first --model-sc superclusters.  No threshold is set: the parity of the bytes is
the criterion.  One JSON line; --out also writes it to a file.

    python tools/matchkind_bench.py [--n-sc 330000] [--model-sc 1500] [--reps 5] [--out profiles/matchkind_bench.json]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sc", type=int, default=330_000)
    ap.add_argument("--model-sc", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    import matchkind_model as MM
    from varstrata_bench import first_superclusters
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api, summary as S
    syn = bench.make_workload(api, args.n_sc, args.seed, "wgs_synth")
    v = syn.variants()
    n_var = [v.n_vars(h) for h in range(4)]
    cls = syn.var_class()
    pr = api.PrecisionRecall()
    res = pr.run(syn.batch(copy=False))
    pb, _, _ = S.phase(res.sc_phase, np.ones(v.n_sc, np.int32))
    plain = S.pr_counts(pr, cls, pb)
    runs, ec_ms = [], []
    for _ in range(args.reps + 1):        # (the first repetition warms up: code objects, allocations)
        t = time.perf_counter()
        counts = pr.matchkind(v, None, pb)
        runs.append(dict(k_matchkind_ms=pr.matchkind_timing(), wall_ms=(time.perf_counter() - t) * 1e3))
        pr.errclass(v, None, pb)
        ec_ms.append(pr.errclass_timing())
    runs, ec_ms = runs[1:], ec_ms[1:]
    ok = bool(np.array_equal(counts[0].sum(1), plain[0, :, A.ERRTYPE_TP]) and np.array_equal(counts[1].sum(1), plain[1, :, A.ERRTYPE_TP]))
    names, specs = api.varstrata_default()
    vs_ms = []
    for _ in range(args.reps + 1):
        pr.varstrata_masks(v, specs)
        vs_ms.append(pr.varstrata_timing())
    vs_ms = vs_ms[1:]
    best, ec_best, vs_best = min(r["k_matchkind_ms"] for r in runs), min(ec_ms), min(vs_ms)
    mk_names = api.matchkind_names()
    largest = int(max(np.diff(v.var_off[h]).max() for h in range(4)))
    out = dict(workload="wgs_synth", n_sc=args.n_sc, hap_variants=int(sum(n_var)), largest_supercluster_variants_per_slot=largest,
               query_tp={n: int(counts[0, 3, c, 0]) for c, n in enumerate(mk_names)}, truth_tp={n: int(counts[1, 3, c, 0]) for c, n in enumerate(mk_names)},
               invariant_holds=ok, k_matchkind_ms=best, hap_variants_per_s=sum(n_var) / (best / 1e3), all_runs=runs,
               beside=dict(k_errclass_ms=ec_best, k_errclass_all_runs=ec_ms, k_varstrata_mask_ms=vs_best, k_varstrata_mask_all_runs=vs_ms),
               matchkind_over_errclass=best / max(ec_best, 1e-9), matchkind_over_varstrata=best / max(vs_best, 1e-9))
    if args.model_sc > 0:
        n = min(args.model_sc, v.n_sc)
        part = first_superclusters(A, v, n)
        nv = [part.n_vars(h) for h in range(4)]
        cut = lambda name: [[getattr(res, name)[h][w][:nv[h]] for w in range(2)] for h in range(4)]
        res_part = types.SimpleNamespace(sc_phase=res.sc_phase[:n], errtype=cut("errtype"), callq=cut("callq"), sync_group=cut("sync_group"),
                                         query_ed=cut("query_ed"))
        t = time.perf_counter()
        want = MM.kinds(part, res_part, pb[:n])
        model_s = time.perf_counter() - t
        pr.matchkind(v, None, pb)
        got = pr.matchkind_download()
        same = all(np.array_equal(got[h][:nv[h]], want[h]) for h in range(4))
        out["model"] = dict(superclusters=n, hap_variants=int(sum(nv)), wall_s=model_s, equal=bool(same),
                            kinds={nm: int(sum((want[h] == c).sum() for h in range(4))) for c, nm in enumerate(mk_names)})
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not ok:
        raise SystemExit("the kinds do not sum to the counters' TP")
    if args.model_sc > 0 and not out["model"]["equal"]:
        raise SystemExit("the device's kind bytes differ from the model's")


if __name__ == "__main__":
    main()
