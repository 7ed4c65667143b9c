"""Regenerates tests/golden/ref/: cases and what the REFERENCE's own functions answer for them (oracle/_ref/ref_harness, built by
`make -C oracle ref` where the reference's sources are at hand).  Seeded and deterministic; refuses to run without the
harness.  tests/ref_pins.py describes the files; tests/golden/README.md the case sets.  Run from the repository's root:
    python tests/golden/make_ref_goldens.py [set ...]          (sets: swg ed cluster chain demo realign window_edges cluster_edges; default: all)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ref_pins as R  # noqa: E402

MAX_FIXTURE_BYTES = 543_000          # the largest file committed before these (tests/golden/demo/query.vcf)
PENALTIES = [(5, 6, 2), (3, 2, 1), (4, 3, 2), (1, 1, 1), (9, 2, 1), (1, 3, 2)]      # ..., x > o + e, x < e
S, I, D = R.TYPE_SUB, R.TYPE_INS, R.TYPE_DEL
DROPPED = {}


def save(name, cmd, case, timeout_s, extra=None):
    """runs the harness on the case and stores inputs + answer; a refusal is stored as such (hand cases are never dropped)"""
    t0 = time.time()
    try:
        out = R.run_harness(cmd, case, timeout=timeout_s)
    except R.Refused as e:
        out = str(e)
        print(f"  {name}: the reference refuses: {out}")
    dt = time.time() - t0
    path = R.save_fixture(name, cmd, case, out, timeout_s, extra)
    size = os.path.getsize(path)
    assert size <= MAX_FIXTURE_BYTES, (name, size)
    print(f"  {name}: {dt:.1f} s, {size} bytes")
    return out


# ---- swg / ed

def mutate(rng, s, rate, letters):
    out = bytearray()
    for c in s:
        if rng.random() < rate:
            k = rng.integers(0, 3)
            if k == 0:
                out.append(letters[rng.integers(0, len(letters))])          # substitution (possibly the same base)
            elif k == 1:
                out.append(c); out.append(letters[rng.integers(0, len(letters))])
            # k == 2: deletion
        else:
            out.append(c)
    return bytes(out) or bytes([letters[0]])


def hand_pairs():
    rng = np.random.default_rng(101)
    flank_a, flank_b = b"ACGTTGCATCAG", b"CTAGGATCCATG"
    p = [(b"ACGTACGTAC", b"ACGTACGTAC"), (b"A", b"A"), (b"A", b"C"), (b"A", b"ACGT"), (b"ACGT", b"A"), (b"A", b"TTTA"), (b"T", b"TAAA"),
         (b"G", b"CCCC"), (b"CCCC", b"G"),
         # one string a prefix / suffix of the other (the trailing-gap rule on reversed strings)
         (b"CCCC", b"CCCCGG"), (b"CCCCGG", b"CCCC"), (b"GGCCCC", b"CCCC"), (b"CCCC", b"GGCCCC"), (b"ACGTAC", b"ACGTACGTACGT"), (b"GTACGTACGT", b"ACGT"),
         # INS and DEL close into one SUB cell
         (b"ACAC", b"CCCAACA"), (b"CCCAACA", b"ACAC"),
         # homopolymer runs: INS-then-DEL and DEL-then-INS tie
         (b"AAAAATTTTT", b"AAAATTTTTT"), (b"CAAAAAG", b"CTTTTTTG"), (b"AAAAAAAAAA", b"AAAAA"), (b"AAAAA", b"AAAAAAAAAA"),
         (b"AAAAAGAAAAA", b"AAAAAAAAAA"), (b"GAAAATTTTC", b"GTTTTAAAAC"), (b"AAAACCCC", b"AAAAGCCCC"), (b"AAAAGCCCC", b"AAAACCCC"),
         (b"TTTTTTTT", b"TTTTATTTT"), (b"CACACACACA", b"ACACACACAC"),
         # a band that touches diagonal 0 and diagonal q + t - 2
         (b"AAAAAAAA", b"TTTTTTTT"), (b"AAAAAAAAAA", b"CCC"), (b"CCC", b"AAAAAAAAAA"), (b"ACGTACGTACGT", b"TGCATGCATGCATGCATGCA")]
    # a substitution run against an insertion + deletion: L x = 2 (o + L e) at L = 12 for 5/6/2, L = 4 for 3/2/1, never for the others
    for L in range(1, 15):
        p.append((flank_a + b"G" * L + flank_b, flank_a + b"T" * L + flank_b))
    # 63, 64, 65, 127, 128, 129 diagonals (q + t - 1): the wavefront kernel strides lanes by 64
    for lq, lt in ((32, 32), (32, 33), (33, 32), (33, 33), (64, 64), (64, 65), (65, 64), (65, 65)):
        q = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), lq))
        t = bytearray(q[:lt].ljust(lt, b"A"))
        for k in rng.choice(lt, 3, replace=False):
            t[k] = b"ACGT"[(b"ACGT".index(t[k]) + 1) % 4]
        p.append((q, bytes(t)))
        p.append((q, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), lt))))      # unrelated: the whole band is used
    return p


def random_pairs(seed, n, letters, max_len=2000):
    rng = np.random.default_rng(seed)
    rates = [0.0, 0.01, 0.03, 0.1, 0.2, 0.3]
    out = []
    for _ in range(n):
        ln = int(np.exp(rng.uniform(0, np.log(max_len))))
        q = bytes(rng.choice(np.frombuffer(letters, np.uint8), ln))
        out.append((q, mutate(rng, q, rates[rng.integers(0, len(rates))], letters)))
    return out


def sv_pairs(seed, n):
    """up to 12 000 bases with one SV-sized gap and a few small edits"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(6000, 12001))
        q = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), ln))
        a = int(rng.integers(100, ln - 2000))
        gap = int(rng.integers(50, 1500))
        t = mutate(rng, q[:a], 0.002, b"ACGT") + (q[a + gap:] if rng.random() < 0.5 else bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), gap)) + q[a:])
        out.append((q, t) if rng.random() < 0.5 else (t, q))
    return out


def save_pairs(name, cmd, pairs, pen, per_case_s, random_set):
    """one fixture of many pairs.  A pair the reference refuses: dropped from a random set (counted, at most 2 %), recorded in
    a fixture of its own for a hand set."""
    case = R.pairs_case(pairs, pen)
    try:
        R.run_harness(cmd, case, timeout=per_case_s * len(pairs))
        kept, refused = pairs, []
    except R.Refused:
        kept, refused = [], []
        for k, pr in enumerate(pairs):
            try:
                R.run_harness(cmd, R.pairs_case([pr], pen), timeout=per_case_s)
                kept.append(pr)
            except R.Refused:
                refused.append((k, pr))
    if random_set:
        assert len(refused) <= 0.02 * len(pairs), (name, len(refused))
        print(f"  {name}: dropped {len(refused)} of {len(pairs)}")
        DROPPED[name] = (len(refused), len(pairs))
    else:
        for k, pr in refused:
            save(f"{name}_refused{k}", cmd, R.pairs_case([pr], pen), per_case_s)
    save(name, cmd, R.pairs_case(kept, pen), per_case_s * max(len(kept), 1), dict(n_dropped=len(refused) if random_set else 0, n_pairs=len(pairs)))


def make_swg():
    hp = hand_pairs()
    for x, o, e in PENALTIES:
        save_pairs(f"swg_hand_{x}{o}{e}", "swg", hp, (x, o, e), 20, False)
    for k, (pen, letters, n) in enumerate([((3, 2, 1), b"ACGT", 700), ((5, 6, 2), b"ACGT", 700), ((3, 2, 1), b"AC", 400), ((5, 6, 2), b"AC", 400),
                                            ((4, 3, 2), b"ACGT", 200), ((1, 1, 1), b"AC", 200), ((9, 2, 1), b"ACGT", 200), ((1, 3, 2), b"AC", 200)]):
        save_pairs(f"swg_random{k}_{pen[0]}{pen[1]}{pen[2]}_{len(letters)}", "swg", random_pairs(200 + k, n, letters), pen, 60, True)
    save_pairs("swg_sv_321", "swg", sv_pairs(300, 6), (3, 2, 1), 120, True)
    save_pairs("swg_sv_562", "swg", sv_pairs(301, 6), (5, 6, 2), 120, True)


def make_ed():
    hp = hand_pairs() + [(b"", b"ACG"), (b"AC", b""), (b"", b"")]
    save_pairs("ed_hand", "ed", hp, (0, 0, 0), 20, False)
    save_pairs("ed_random_4", "ed", random_pairs(400, 1500, b"ACGT"), (0, 0, 0), 60, True)
    save_pairs("ed_random_2", "ed", random_pairs(401, 800, b"AC"), (0, 0, 0), 60, True)
    # lengths across 64, 4 096 and 65 536 at a small distance (wf_ed is a wavefront: long and similar is cheap)
    rng = np.random.default_rng(402)
    pairs = []
    for n in (63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537):
        q = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
        t = bytearray(q)
        for k in sorted(rng.choice(n - 2, 5, replace=False), reverse=True):
            op = int(rng.integers(0, 3))
            if op == 0:
                t[k] = b"ACGT"[(b"ACGT".index(t[k]) + 1) % 4]
            elif op == 1:
                t.insert(k, b"ACGT"[int(rng.integers(0, 4))])
            else:
                del t[k]
        pairs += [(q, bytes(t)), (bytes(t), q), (q, q[:-1]), (q[1:], q)]
    save_pairs("ed_crossing", "ed", pairs, (0, 0, 0), 120, True)


# ---- chain

def variants_to_case(v, args, per_sc=False, pad=64, phase_sets=None):
    """an A.Variants as a chain case.  per_sc: every supercluster becomes a contig of its own (its region with `pad` bases of the
    neighbourhood on either side), which keeps a synthetic batch's superclusters apart whatever the clustering gap"""
    contigs, sites = [], [[] for _ in range(4)]
    if per_sc:
        for sc in range(v.n_sc):
            c0, c1 = int(v.ctg_off[v.sc_ctg[sc]]), int(v.ctg_off[v.sc_ctg[sc] + 1])
            a = max(int(v.sc_beg[sc]) - pad, 0)
            b = min(int(v.sc_end[sc]) + 1 + pad, c1 - c0)
            contigs.append((f"s{sc:04d}", bytes(v.ctg_seq[c0 + a:c0 + b])))
            for h in range(4):
                for i in range(int(v.var_off[h][sc]), int(v.var_off[h][sc + 1])):
                    sites[h].append((sc, int(v.var_pos[h][i]) - a, i))
    else:
        for c in range(len(v.ctg_off) - 1):
            contigs.append((f"chr{c + 1}", bytes(v.ctg_seq[int(v.ctg_off[c]):int(v.ctg_off[c + 1])])))
        for h in range(4):
            for sc in range(v.n_sc):
                for i in range(int(v.var_off[h][sc]), int(v.var_off[h][sc + 1])):
                    sites[h].append((int(v.sc_ctg[sc]), int(v.var_pos[h][i]), i))
    slots = []
    for h in range(4):
        pool = bytes(v.allele_pool[h])
        rows = []
        for c, pos, i in sites[h]:
            ref = pool[int(v.var_ref_off[h][i]):int(v.var_ref_off[h][i]) + int(v.var_ref_len[h][i])]
            alt = pool[int(v.var_alt_off[h][i]):int(v.var_alt_off[h][i]) + int(v.var_alt_len[h][i])]
            rows.append((c, pos, int(v.var_type[h][i]), ref, alt, float(v.var_qual[h][i]), 0 if phase_sets is None else int(phase_sets[h][i])))
        slots.append(R.slot_from_sites(rows))
    return R.chain_case(contigs, slots, args)


def limit_variants(k):
    """tests/test_gpu_distance.py's _limit_batch with k directly adjacent one-base deletion records in the middle supercluster"""
    from vcfdist_amd import _abi as A
    rng = np.random.RandomState(23)
    ref = "".join(rng.choice(list("ACGT"), 400))
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    run = [(200 + j, D, ref[200 + j], "", 30.0) for j in range(k)]
    scs = [dict(ctg=0, beg=40, end=70, vars=[[(50, S, ref[50], other(ref[50]), 20.0)], [], [(50, S, ref[50], other(ref[50]), 40.0)],
                                             [(60, I, "", "GT", 9.0)]]),
           dict(ctg=0, beg=190, end=220, vars=[run, [], [(200, D, ref[200:200 + k], "", 50.0)], []]),
           dict(ctg=0, beg=300, end=340, vars=[[(310, D, ref[310:313], "", 20.0)], [(320, S, ref[320], other(ref[320]), 5.0)],
                                               [(310, D, ref[310:313], "", 40.0)], [(320, S, ref[320], other(ref[320]), 7.0)]])]
    return A.Variants.from_sites([ref], scs)


BASE = ["-t", "4", "-v", "0", "-n", "-d"]
GAP50 = ["-c", "gap", "50"]


def make_chain():
    from vcfdist_amd import api
    import make_regression as MR
    import test_oracle as TO
    import indel_runs
    # (a) the regression batches' shapes, two further seeds of each, one contig per synthetic supercluster
    for tag, params, seeds in (("seed", MR.PARAMS, (7, 107, 207)), ("joint", MR.PARAMS_JOINT, (61, 161, 261))):
        for seed, cl in zip(seeds, (GAP50, ["-c", "gap", "200"], ["-c", "biwfa"])):
            v = api.Synth(**dict(params, seed=seed)).variants()
            save(f"chain_{tag}{seed}", "chain", variants_to_case(v, cl + BASE, per_sc=True), 600)
    # (b) hand cases
    save("chain_toy", "chain", variants_to_case(TO.toy_variants(), GAP50 + BASE), 60)
    for k, hc in enumerate(TO.HAND_CASES):
        save(f"chain_hand{k}", "chain", variants_to_case(TO.hand_case_variants(hc), GAP50 + BASE), 60)
    for k in (7, 8, 9, 12):
        save(f"chain_limit{k}", "chain", variants_to_case(limit_variants(k), GAP50 + BASE), 60)
    # swap-predecessor ties that the tie replay exists for: the smoke batch's shape (more superclusters and another seed: with the
    # reference's own regions the 64 of seed 7 hold no tie decided other than 'largest source') and test_gpu_parity's tiny_repeats
    v = api.Synth(n_sc=320, len_a=8, len_b=300, len_max=300, seed=8, var_per_base=0.03).variants()
    save("chain_ties_smoke", "chain", variants_to_case(v, ["-c", "gap", "200"] + BASE, per_sc=True), 300)
    v = api.Synth(n_sc=400, len_a=6, len_b=60, len_min=5, len_max=60, seed=1, var_per_base=0.08, p_snp=0.5, p_repeat=0.5).variants()
    save("chain_ties_tiny", "chain", variants_to_case(v, ["-c", "gap", "200"] + BASE, per_sc=True), 300)
    # runs of directly adjacent deletion records: many allowed swap sources on one position
    save("chain_runs", "chain", variants_to_case(indel_runs.indel_run_superclusters(21, n_sc=40), ["-c", "gap", "20"] + BASE), 300)
    # superclusters at position 0 / 1 and at a contig's end, a contig in one callset only, empty haplotypes, phase sets
    rng = np.random.RandomState(77)
    seqs = ["".join(rng.choice(list("ACGT"), n)) for n in (300, 240, 200, 260)]
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    snp = lambda c, p, q, ps=0: (c, p, S, seqs[c][p], other(seqs[c][p]), q, ps)
    for name, slots, qc, tc in (
            ("chain_edges_pos0", [[snp(0, 0, 20.0), snp(0, 150, 21.0)], [snp(0, 150, 21.0)], [snp(0, 0, 30.0)], [snp(0, 150, 31.0)]], None, None),
            ("chain_edges_pos1", [[snp(0, 1, 20.0), (0, 120, D, seqs[0][120:123], "", 22.0)], [], [snp(0, 1, 30.0)], [(0, 120, D, seqs[0][120:123], "", 32.0)]], None, None),
            ("chain_edges_end", [[snp(0, 297, 20.0)], [(0, 290, I, "", "GT", 12.0)], [snp(0, 297, 30.0), (0, 280, D, seqs[0][280:284], "", 9.0)][::-1], []], None, None),
            ("chain_edges_last_base", [[snp(0, 299, 20.0)], [], [snp(0, 299, 30.0)], []], None, None),
            ("chain_one_callset_contig", [[snp(0, 50, 20.0), snp(1, 60, 21.0), snp(3, 30, 5.0)], [snp(1, 60, 21.0)],
                                          [snp(0, 50, 30.0), snp(2, 70, 31.0)], [snp(2, 90, 32.0)]], [0, 1, 3], [0, 2]),
            ("chain_empty_haps", [[], [], [snp(0, 50, 30.0)], []], None, None),
            ("chain_no_variants", [[], [], [], []], None, None),
            ("chain_phase_sets", [[snp(0, 40, 20.0, 41), snp(0, 200, 21.0, 201)], [snp(1, 100, 22.0, 101)], [snp(0, 200, 30.0, 41)], [snp(0, 40, 31.0, 41), snp(1, 100, 32.0, 101)]],
             None, None)):
        case = R.chain_case([(f"chr{k + 1}", s.encode()) for k, s in enumerate(seqs)], [R.slot_from_sites(s) for s in slots], GAP50 + BASE, qc, tc)
        save(name, "chain", case, 60)


def window_edge_cases():
    """the subset of tests/window_edge_cases.py's table behind chain_window_edges: the two cases on either side of every border
    of the 16- and the 64-cell level (shift at distance 0, priced with one mutation; both signs), the priced ties, and two cases
    each whose paths need the 256-cell, the 1024-cell and the dense level (deletion forms at 1024: haplotypes below 2 000 bases)"""
    import window_edge_cases as WE
    needs = WE.needs(WE.TABLE)
    sweep = {}
    for c in WE.TABLE:
        if (c.family == "shift" and c.snp == 0 and c.form == "ins") or (c.family == "priced" and c.k == 1):
            sweep[(c.family, c.sign, c.u)] = c
    out = []
    for (fam, sign, u), c in sweep.items():
        up = sweep.get((fam, sign, u + 1))
        lv = needs[c.name][0].level
        if up is not None and lv in (16, 64) and needs[up.name][0].level == WE.next_level(lv):
            out += [c, up]
    assert len(out) == 2 * 2 * 2 * 2, len(out)
    out += [c for c in WE.TABLE if c.tie]
    for lv in (256, 1024, WE.DENSE):
        fit = [c for c in WE.TABLE if c.family == "shift" and c.W == 1024 // (4 if lv == 256 else 1) and c.snp < 2 and
               (c.form == "del" or lv == 256) and needs[c.name][0].level == lv]
        out += fit[:2] if lv == WE.DENSE else fit[-2:]          # (the ones next to the border)
    assert len(out) == 16 + 6 + 6 and len({c.name for c in out}) == len(out), [c.name for c in out]
    assert all(max(needs[c.name][0].lens) < 2000 for c in out)
    return out


def make_window_edges():
    """paths along the edge of a window level (tests/window_edge_cases.py).  `-c gap 2000` keeps a case's two variants, a whole
    tract apart, in one supercluster; every case is a contig of its own"""
    import window_edge_cases as WE
    cases = window_edge_cases()
    v, _, _ = WE.batch_of(cases)
    save("chain_window_edges", "chain", variants_to_case(v, ["-c", "gap", "2000"] + BASE, per_sc=True), 600,
         extra=dict(case_names=np.frombuffer("\n".join(c.name for c in cases).encode(), np.uint8)))


def make_cluster():
    """clustering alone, on whole synthetic contigs (no precision/recall behind it, so the clusters may grow large): the size
    method, and wf_swg_cluster at other penalties and iteration limits"""
    from vcfdist_amd import api
    import make_regression as MR
    import test_gpu_realign as TR
    base = ["-t", "4", "-v", "0", "-n"]
    vj = api.Synth(**MR.PARAMS_JOINT).variants()
    vs = api.Synth(**MR.PARAMS).variants()
    vw = api.Synth(**dict(TR.WGS, n_sc=3000)).variants()
    for name, v, args in (("cluster_size50_joint", vj, ["-c", "size", "50"]), ("cluster_size10_seed", vs, ["-c", "size", "10"]),
                          ("cluster_gap10_seed", vs, ["-c", "gap", "10"]), ("cluster_gap50_wgs", vw, GAP50),
                          ("cluster_biwfa_seed_321", vs, ["-c", "biwfa", "-x", "3", "-o", "2", "-e", "1"]),
                          ("cluster_biwfa_seed_i1", vs, ["-c", "biwfa", "-i", "1"]), ("cluster_biwfa_wgs", vw, ["-c", "biwfa"])):
        save(name, "cluster", variants_to_case(v, args + base), 600)


def cluster_edge_case(cases, pen, itrs):
    """cases of tests/wfa_cluster_cases.py as one cluster case: a contig per case, its variants as query hap 1"""
    sites = [(ci, p, t, r, a, 30.0) for ci, c in enumerate(cases) for p, t, r, a in c.variants]
    args = ["-c", "biwfa", "-x", str(pen[0]), "-o", str(pen[1]), "-e", str(pen[2]), "-i", str(itrs), "-t", "4", "-v", "0", "-n"]
    return R.chain_case([(c.name, c.ctg.encode()) for c in cases], [R.slot_from_sites(sites)] + [R.empty_slot()] * 3, args)


def make_cluster_edges():
    """tests/wfa_cluster_cases.py: the biWFA clustering at its size classes, lane chunks, ring length, doubling rounds, contig ends
    and merge passes.  One fixture per penalty set and iteration limit (the arguments are per fixture); a case of undefined input
    is a fixture of its own, `_refused` where the reference refuses it"""
    import wfa_cluster_cases as WC
    names = lambda cases: dict(case_names=np.frombuffer("\n".join(c.name for c in cases).encode(), np.uint8))
    for (pen, itrs), cases in sorted(WC.fixture_sets().items()):
        out = save(WC.fixture_name(pen, itrs), "cluster", cluster_edge_case(cases, pen, itrs), 300, extra=names(cases))
        assert not isinstance(out, str), out
    for c in WC.UNDEFINED:
        case = cluster_edge_case([c], c.pen, c.itrs[0])
        try:
            R.run_harness("cluster", case, timeout=60)
            tail = ""
        except R.Refused:
            tail = "_refused"
        save("cluster_biwfa_edges_" + c.name[len("edge_"):] + tail, "cluster", case, 60, extra=names([c]))


def demo_case(args):
    import demo_pipeline as DP
    from vcfdist_amd import io as IO
    bed = IO.Bed(os.path.join(DP.DEMO, "nist-v4.2.1_chr1_5Mb.bed"))
    sets = [IO.read_vcf(os.path.join(DP.DEMO, f), bed) for f in ("query.vcf", "nist-v4.2.1_chr1_5Mb.vcf.gz")]
    slots = []
    for cs in sets:
        assert cs["contigs"] == ["chr1"]
        for s in cs["vars"][0]:
            pool = bytes(s["pool"])
            n = len(s["pos"])
            slots.append(dict(ctg=[0] * n, pos=s["pos"], rlen=s["rlen"], type=s["type"], var_qual=s["var_qual"], gt_qual=s.get("gt_qual", []),
                              orig_gt=s.get("orig_gt", []), phase_set=s["phase_set"], loc=[],
                              ref=[pool[int(o):int(o) + int(l)] for o, l in zip(s["ref_off"], s["ref_len"])],
                              alt=[pool[int(o):int(o) + int(l)] for o, l in zip(s["alt_off"], s["alt_len"])]))
    return R.chain_case([("chr1", bytes(DP.surrogate_fasta(5_100_000)))], slots, args)


def make_demo():
    """the demo's variants as vcfdist_amd.io.read_vcf reads them, on the seeded surrogate FASTA (rebuilt by the tests, not stored)"""
    for tag, cl in (("gap50", GAP50), ("gap200", ["-c", "gap", "200"]), ("biwfa", ["-c", "biwfa"])):
        for d in ("", "-d"):
            case = demo_case(cl + ["-t", "4", "-v", "0", "-n"] + ([d] if d else []))
            seq = case.pop("ctg_seq")
            t0 = time.time()
            out = R.run_harness("chain", dict(case, ctg_seq=seq), timeout=1800)
            path = R.save_fixture(f"demo_{tag}{'_d' if d else ''}", "chain", case, out, 1800, dict(surrogate_len=len(seq)))
            print(f"  demo_{tag}{d}: {time.time() - t0:.1f} s, {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= MAX_FIXTURE_BYTES


# ---- realign

def realign_case(callsets, args):
    """callsets: tests/test_gpu_realign.py's (hap, clusters, contig) per contig -> a realign case with the haps as query hap 1"""
    contigs, rows = [], R.empty_slot()
    for c, (hap, cl, seq) in enumerate(callsets):
        contigs.append((f"chr{c + 1}", bytes(seq)))
        pool = bytes(hap["pool"])
        for i in range(len(hap["pos"])):
            rows["ctg"].append(c); rows["pos"].append(int(hap["pos"][i])); rows["type"].append(int(hap["type"][i])); rows["rlen"].append(int(hap["rlen"][i]))
            rows["ref"].append(pool[int(hap["ref_off"][i]):int(hap["ref_off"][i]) + int(hap["ref_len"][i])])
            rows["alt"].append(pool[int(hap["alt_off"][i]):int(hap["alt_off"][i]) + int(hap["alt_len"][i])])
            rows["var_qual"].append(float(hap["var_qual"][i])); rows["gt_qual"].append(float(hap["gt_qual"][i]))
            rows["orig_gt"].append(int(hap["orig_gt"][i])); rows["phase_set"].append(int(hap["phase_set"][i])); rows["loc"].append(R.BED_INSIDE)
    return R.chain_case(contigs, [rows, R.empty_slot(), R.empty_slot(), R.empty_slot()], args)


def make_realign():
    import test_gpu_realign as TR
    base = ["-t", "4", "-v", "0", "-n", "-rq"]
    save("realign_wgs", "realign", realign_case(TR.callsets(dict(TR.WGS, n_sc=10000)), GAP50 + base), 600)
    save("realign_joint", "realign", realign_case(TR.callsets(TR.JOINT), GAP50 + base), 900)
    save("realign_joint_321", "realign", realign_case(TR.callsets(dict(TR.JOINT, n_sc=400)), GAP50 + base + ["-x", "3", "-o", "2", "-e", "1", "-mx", "40"]), 600)
    # hand cases: a cluster at position 1 (the region starts one base before its first variant), a cluster whose region passes
    # the contig's end, adjacent INS + DEL that left_shift moves, a homopolymer where left-shifting meets another record
    seq = "GATTACAGCCTGCAAAAAAGTAGCATCGGATCTTGACCATTTTTTTTGCAGCATCAGCAGCAGCAGCTTAGC"
    n = len(seq)
    for name, sites in (("realign_hand_pos1", [(0, 1, S, seq[1], "C", 30.0, 7), (0, 3, D, seq[3:5], "", 20.0, 7)]),
                        ("realign_hand_pos0", [(0, 0, S, seq[0], "C", 30.0, 7)]),
                        ("realign_hand_end", [(0, n - 3, D, seq[n - 3:n - 1], "", 30.0), (0, n - 1, S, seq[n - 1], "A", 25.0)]),
                        ("realign_hand_last", [(0, n - 2, D, seq[n - 2:], "", 30.0)]),
                        ("realign_hand_ins_del", [(0, 20, I, "", "A", 30.0), (0, 20, D, seq[20:22], "", 31.0), (0, 45, D, "T", "", 12.0)]),
                        ("realign_hand_overlap", [(0, 22, D, seq[22:26], "", 30.0), (0, 24, S, seq[24], "T", 31.0)]),
                        ("realign_hand_homopolymer", [(0, 13, S, "A", "G", 40.0), (0, 18, D, "A", "", 30.0), (0, 46, I, "", "TT", 22.0), (0, 47, S, "T", "C", 9.0),
                                                      (0, 60, D, "CAG", "", 33.0, 5)])):
        save(name, "realign", R.chain_case([("chr1", seq.encode())], [R.slot_from_sites(sites)] + [R.empty_slot()] * 3, GAP50 + base), 60)


SETS = {"swg": make_swg, "ed": make_ed, "cluster": make_cluster, "chain": make_chain, "demo": make_demo, "realign": make_realign,
        "window_edges": make_window_edges, "cluster_edges": make_cluster_edges}          # (chain_window_edges: a set of its own, it computes needed_level for the whole table)


def main(argv):
    if not R.have_harness():
        raise SystemExit("oracle/_ref/ref_harness is missing: build it with `make -C oracle ref` (needs the reference's sources)")
    for name in argv or list(SETS):
        print(name)
        SETS[name]()
    for name, (d, n) in DROPPED.items():
        print(f"dropped {d} of {n} in {name}")


if __name__ == "__main__":
    main(sys.argv[1:])
