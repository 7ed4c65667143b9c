"""Times vpr_context_masks (--stratify-context, include/vcfdist_context.h) with the default set on one synthetic contig of 50 Mb
(seeded random bases with the default strata's tracts planted, so that no stratum is empty) and a million synthetic variants:
device ms of the interval kernels and of the membership kernel (HIP events, the best of --reps calls), bases/s, and the
bandwidth that figure implies for the bytes the passes have to move -- per stratum one read of the sequence (1 byte per base),
one write and one read of the flag bits (1/8 byte each) -- beside the HBM figures of the MI355X.  Beside it the numpy model
(tests/context_model.py) on a 5 Mb slice of the same contig, whose intervals the GPU's on that slice must equal.  One JSON line;
--out also writes it to a file.

    python tools/context_bench.py [--bases 50000000] [--model-bases 5000000] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_SPEC_TBS, HBM_MEASURED_TBS = 8.0, 6.29       # MI355X: HBM3E peak, and a float4 copy


def make_contig(n, seed):
    import context_cases as CC
    rng = np.random.RandomState(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)
    for i, pos in enumerate(range(10_000, n - 10_000, 100_000)):      # every default stratum's tract, over and over along the contig
        CC.plant_at(seq, pos, i % 11, rng)
    return seq


def make_variants(A, seq, n_sc, seed):
    """n_sc superclusters with one substitution per hap slot each, at sorted random positions"""
    rng = np.random.RandomState(seed)
    pos = [np.sort(rng.randint(0, len(seq), n_sc)).astype(np.int32) for _ in range(4)]
    off = np.arange(n_sc + 1, dtype=np.int64)
    one, z = np.ones(n_sc, np.int32), np.zeros(n_sc, np.int32)
    return A.Variants(np.array([0, len(seq)], np.int64), seq, z, z, one, [off] * 4, pos, [np.full(n_sc, A.TYPE_SUB, np.uint8)] * 4,
                      [np.full(n_sc, 30, np.float32)] * 4, [np.arange(n_sc, dtype=np.int64)] * 4, [one] * 4, [np.arange(n_sc, dtype=np.int64)] * 4,
                      [one] * 4, [np.full(n_sc + 1, 65, np.uint8)] * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--model-bases", type=int, default=5_000_000)
    ap.add_argument("--variants", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import context_model as CM
    from vcfdist_amd import _abi as A
    from vcfdist_amd import api
    names, specs = api.context_default()
    seq = make_contig(args.bases, args.seed)
    v = make_variants(A, seq, args.variants // 4, args.seed + 1)
    pr = api.PrecisionRecall()
    pr.context_masks(v, specs)                      # warm-up: code objects, scan workspaces
    runs = []
    for _ in range(args.reps):
        t = time.perf_counter()
        pr.context_masks(v, specs)
        wall = time.perf_counter() - t
        ms_iv, ms_mask = pr.context_timing()
        runs.append(dict(ms_intervals=ms_iv, ms_mask=ms_mask, wall_ms=wall * 1e3))
    best = min(runs, key=lambda r: r["ms_intervals"])
    rows = pr.download_context_intervals()
    n_iv = {n: int(len(r[0][0])) for n, r in zip(names, rows)}
    assert all(n_iv.values()), n_iv
    words = pr.download_strata_masks()
    members = [int(sum(int(((w[0] >> np.uint64(k)) & np.uint64(1)).sum()) for w in words)) for k in range(len(specs))]
    moved = len(specs) * args.bases * 1.25
    out = dict(bases=args.bases, strata=len(specs), variants=int(sum(v.n_vars(h) for h in range(4))), intervals=n_iv, members=members,
               best=best, all_runs=runs, bases_per_s=args.bases / (best["ms_intervals"] / 1e3),
               stratum_bases_per_s=len(specs) * args.bases / (best["ms_intervals"] / 1e3), bytes_moved_model=moved,
               effective_tb_per_s=moved / (best["ms_intervals"] / 1e3) / 1e12, hbm_spec_tb_per_s=HBM_SPEC_TBS,
               hbm_measured_copy_tb_per_s=HBM_MEASURED_TBS)
    if args.model_bases > 0:
        k = min(args.model_bases, args.bases)
        part = np.ascontiguousarray(seq[:k])
        t = time.perf_counter()
        want = CM.all_intervals([part], specs)
        model_s = time.perf_counter() - t
        pr.context_masks(make_variants(A, part, 4, 3), specs)
        bad = CM.same(pr.download_context_intervals(), want)
        assert not bad, bad
        out["numpy_model"] = dict(bases=k, wall_s=model_s, bases_per_s=k / model_s, gpu_ms_same_slice=pr.context_timing()[0], equal=True)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
