"""Times vpr_derive_masks (--stratify-derive / --stratify-cross, include/vcfdist_derive.h) on the batch of profiles/errclass_bench.json
(wgs_synth, about a million hap-variants) with the default context and variant strata resident: the device time of the k_derive_mask
launches (HIP events on the handle's stream, the best of --reps calls) for three workloads -- the one entry easy=!*, the 154-pair
cross of the variant with the context strata, 512 random entries.  Beside it, in the same run, k_varstrata_mask and k_strata_mask on
the same variants, and a plain device copy of as many bytes as the kernel's lanes load and store (the one-word cache simulated on the
host).  The gate is correctness: the bits of the first --model-vars hap-variants (a quarter per slot) equal the model of
tests/derive_model.py.  No time is set.  One JSON line; --out also writes it to a file.

    python tools/derive_bench.py [--n-sc 330000] [--model-vars 4480] [--reps 5] [--out profiles/derive_bench.json]"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def traffic(code_off, code, n_prev):
    """(words loaded, words stored) per lane: k_derive_mask's accumulator and one-word cache, replayed"""
    cur, cache, loads, stores = n_prev >> 6, -1, 1 if n_prev & 63 else 0, 1
    for j in range(len(code_off) - 1):
        k = n_prev + j
        if k >> 6 != cur:
            cur, stores = k >> 6, stores + 1
        for c in code[code_off[j]:code_off[j + 1]]:
            if c >= 0 and c >> 6 != cur and c >> 6 != cache:
                cache, loads = c >> 6, loads + 1
    return loads, stores


def copy_ms(torch, n_bytes, reps):
    """ms of a device copy that reads n_bytes / 2 and writes n_bytes / 2, the best of reps"""
    a = torch.zeros(max(n_bytes // 16, 1), dtype=torch.int64, device="cuda")
    b = torch.empty_like(a)
    best = float("inf")
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def registers():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "^k_derive_mask$"], capture_output=True, text=True).stdout
    m = re.search(r"vgpr\s+(\d+) sgpr\s+(\d+) lds\s+(\d+) scratch\s+(\d+)", out)
    return dict(zip(("vgpr", "sgpr", "lds", "scratch"), map(int, m.groups()))) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sc", type=int, default=330_000)
    ap.add_argument("--model-vars", type=int, default=4480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch        # (before the library opens the GPU: its HIP runtime is then the process's only one)
    import bench
    import derive_cases as DC
    import derive_model as DM
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api
    v = bench.make_workload(api, args.n_sc, args.seed, "wgs_synth").variants()
    n_var = [v.n_vars(h) for h in range(4)]
    ctx_names, ctx = api.context_default()
    vs_names, vs = api.varstrata_default()
    names = ctx_names + vs_names
    n_prev = len(names)
    pr = api.PrecisionRecall()
    beside = dict(k_strata_mask_ms=[], k_varstrata_mask_ms=[])
    for _ in range(args.reps + 1):        # (the first repetition warms up: code objects, allocations)
        pr.context_masks(v, ctx)
        beside["k_strata_mask_ms"].append(pr.context_timing()[1])
        pr.varstrata_masks(v, vs, append=True)
        beside["k_varstrata_mask_ms"].append(pr.varstrata_timing())
    base = pr.download_strata_masks()
    rng = np.random.RandomState(args.seed)
    pairs = api.derive_cross(",".join(vs_names) + ":" + ",".join(ctx_names), names)
    random_entries = [DC.random_program(rng, n_prev + j) for j in range(512)]
    workloads = (("easy", [list(api.derive_compile("easy=!*", names)[1])]), ("cross_154", [[a, b, A.DV_AND] for a, b in pairs]),
                 ("random_512", random_entries))
    part = args.model_vars // 4
    out = dict(workload="wgs_synth", n_sc=args.n_sc, hap_variants=int(sum(n_var)), resident_strata=n_prev, registers=registers(),
               beside={k: min(ms[1:]) for k, ms in beside.items()}, beside_all_runs={k: ms[1:] for k, ms in beside.items()}, workloads={})
    equal = True
    for name, entries in workloads:
        off = np.cumsum([0] + [len(e) for e in entries]).astype(np.int32)
        code = np.asarray([c for e in entries for c in e], np.int32)
        runs = []
        for _ in range(args.reps + 1):
            pr.upload_strata_masks(n_prev, base)
            pr.derive_masks(off, code)
            runs.append(pr.derive_timing())
        runs = runs[1:]
        got = pr.download_strata_masks()
        n_new = n_prev + len(entries)
        same = all(np.array_equal(DM.bits_of(got[h][:, :part], n_new), DM.run_programs(off, code, DM.bits_of(base[h][:, :part], n_prev))) for h in range(4))
        equal = equal and same
        loads, stores = traffic(off, code, n_prev)
        n_bytes = 8 * (loads + stores) * int(sum(n_var))
        best, cp = min(runs), copy_ms(torch, n_bytes, args.reps)
        members = int(sum(int(((got[h][(n_new - 1) >> 6] >> np.uint64((n_new - 1) & 63)) & np.uint64(1)).sum()) for h in range(4)))
        out["workloads"][name] = dict(entries=len(entries), code_ints=int(len(code)), k_derive_mask_ms=best, all_runs=runs, words_loaded_per_variant=loads,
                                      words_stored_per_variant=stores, bytes_moved=n_bytes, gb_per_s=n_bytes / (best * 1e6), copy_same_bytes_ms=cp,
                                      derive_over_copy=best / max(cp, 1e-9), stack_steps=int(len(code)) * int(sum(n_var)),
                                      stack_steps_per_ns=len(code) * sum(n_var) / (best * 1e6), members_of_last_entry=members, model_equal=bool(same))
    out["model"] = dict(hap_variants=4 * part, equal=bool(equal))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit("the device's membership words differ from the model's")


if __name__ == "__main__":
    main()
