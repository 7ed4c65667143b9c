"""Times vpr_errclass (--classify-errors, include/vcfdist_errclass.h) on an evaluated wgs_synth-shaped batch of about a million
hap-variants (the batch of tools/varstrata_bench.py): the device time of the k_errclass launches (HIP events on the handle's stream,
the best of --reps calls).  Beside it, in the same run and on the same batch, the two kernels it stands beside: the whole
vpr_pr_counts call (host wall time around k_pr_hist: the call has no events of its own) and the k_varstrata_mask launches of the
default variant strata; and the brute-force model (tests/errclass_model.py) on the first --model-sc superclusters, whose classes the
GPU's on that slice must equal.  No threshold is set.  One JSON line; --out also writes it to a file.

    python tools/errclass_bench.py [--n-sc 330000] [--model-sc 1500] [--reps 5] [--out profiles/errclass_bench.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sc", type=int, default=330_000)
    ap.add_argument("--model-sc", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    import errclass_model as EM
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
    runs, hist_ms = [], []
    for _ in range(args.reps + 1):        # (the first repetition warms up: code objects, allocations)
        t = time.perf_counter()
        counts = pr.errclass(v, None, pb, args.window)
        runs.append(dict(k_errclass_ms=pr.errclass_timing(), wall_ms=(time.perf_counter() - t) * 1e3))
        t = time.perf_counter()
        S.pr_counts(pr, None, pb)
        hist_ms.append((time.perf_counter() - t) * 1e3)
    runs, hist_ms = runs[1:], hist_ms[1:]
    ok = bool(np.array_equal(counts[0].sum(1), plain[0, :, A.ERRTYPE_FP]) and np.array_equal(counts[1].sum(1), plain[1, :, A.ERRTYPE_FN]))
    names, specs = api.varstrata_default()
    vs_ms = []
    for _ in range(args.reps + 1):
        pr.varstrata_masks(v, specs)
        vs_ms.append(pr.varstrata_timing())
    vs_ms = vs_ms[1:]
    best, vs_best = min(r["k_errclass_ms"] for r in runs), min(vs_ms)
    ec_names = api.errclass_names()
    out = dict(workload="wgs_synth", n_sc=args.n_sc, hap_variants=int(sum(n_var)), window=args.window,
               query_fp={n: int(counts[0, 3, c, 0]) for c, n in enumerate(ec_names[:6])}, truth_fn={n: int(counts[1, 3, c, 0]) for c, n in enumerate(ec_names)},
               truth_fn_at_max_qual={n: int(counts[1, 3, c, -1]) for c, n in enumerate(ec_names)}, invariant_holds=ok,
               k_errclass_ms=best, hap_variants_per_s=sum(n_var) / (best / 1e3), all_runs=runs,
               beside=dict(vpr_pr_counts_wall_ms=min(hist_ms), vpr_pr_counts_all_runs=hist_ms, k_varstrata_mask_ms=vs_best, k_varstrata_mask_all_runs=vs_ms),
               errclass_over_varstrata=best / max(vs_best, 1e-9))
    if args.model_sc > 0:
        n = min(args.model_sc, v.n_sc)
        part = first_superclusters(A, v, n)
        nv = [part.n_vars(h) for h in range(4)]
        res_part = types.SimpleNamespace(sc_phase=res.sc_phase[:n], errtype=[[res.errtype[h][w][:nv[h]] for w in range(2)] for h in range(4)],
                                         callq=[[res.callq[h][w][:nv[h]] for w in range(2)] for h in range(4)])
        t = time.perf_counter()
        want = EM.classes(part, res_part, pb[:n], args.window)
        model_s = time.perf_counter() - t
        pr.errclass(v, None, pb, args.window)
        got = pr.errclass_download()
        same = all(np.array_equal(got[h][:nv[h]], want[h]) for h in range(4))
        out["model"] = dict(superclusters=n, hap_variants=int(sum(nv)), wall_s=model_s, hap_variants_per_s=sum(nv) / model_s, equal=bool(same))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not ok:
        raise SystemExit("the classes do not sum to the counters' FP / FN")
    if args.model_sc > 0 and not out["model"]["equal"]:
        raise SystemExit("the device's class bytes differ from the model's")


if __name__ == "__main__":
    main()
