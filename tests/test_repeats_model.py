"""The numpy model of the repeat strata (tests/repeats_model.py) against a brute-force restatement of the definitions, the C
ABI's declarations, and the conditions the GPU tests' inputs (tests/repeats_cases.py) have to meet for those tests not to pass
vacuously."""
import os
import re

import numpy as np
import pytest

import repeats_cases as RC
import repeats_model as RM
from vcfdist_amd import _abi as A
from vcfdist_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definitions once more, written separately: all pairs of starts, string comparison, an explicit reverse complement

def brute_intervals(contigs, k, slop):
    """-> (rows[contig] = [(start, stop)], valid starts, repeated starts) straight from include/vcfdist_repeats.h"""
    contigs = [bytes(c).decode() for c in contigs]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    valid = [(c, i) for c, s in enumerate(contigs) for i in range(len(s) - k + 1) if all(ch in "ACGT" for ch in s[i:i + k])]
    word = {(c, i): contigs[c][i:i + k] for c, i in valid}
    rc = {ci: "".join(comp[ch] for ch in reversed(w)) for ci, w in word.items()}
    rep = {ci for ci in valid if any(o != ci and (word[o] == word[ci] or word[o] == rc[ci]) for o in valid)}
    rows = []
    for c, s in enumerate(contigs):
        L, tracts, i = len(s), [], 0
        while i < L:
            if (c, i) in rep:
                a = i
                while (c, i) in rep:
                    i += 1
                tracts.append((max(0, a - slop), min(L, i - 1 + k + slop)))
            else:
                i += 1
        merged = []
        for a, b in tracts:
            if merged and a <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        rows.append(merged)
    return rows, len(valid), len(rep)


def as_pairs(row):
    return [(int(a), int(b)) for a, b in zip(*row)]


def model_equals_brute(contigs, k, slop):
    rows, nv, nr = RM.all_intervals(contigs, [A.rep_kmer(k, slop)])
    want, wv, wr = brute_intervals(contigs, k, slop)
    assert [as_pairs(r) for r in rows[0]] == want and (int(nv[0]), int(nr[0])) == (wv, wr), (k, slop, contigs)
    return want, wv, wr


@pytest.mark.parametrize("k", RC.HAND_K)
def test_model_equals_brute_force_on_hand_cases(k):
    for name, contigs in RC.hand_cases(k).items():
        for slop in (0, 3):
            model_equals_brute(contigs, k, slop)


@pytest.mark.parametrize("k", [4, 5, 8])
def test_model_equals_brute_force_on_random_genomes(k):
    rng = np.random.RandomState(k)
    for t in range(12):
        n_ctg = int(rng.randint(1, 5))
        cuts = np.sort(rng.randint(0, 401, size=n_ctg - 1)) if n_ctg > 1 else np.zeros(0, int)
        total = int(rng.randint(0, 401))
        cuts = np.minimum(cuts, total)
        s = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=total, p=[0.28, 0.22, 0.22, 0.25, 0.03]))
        contigs = [s[a:b] for a, b in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [total])))]
        model_equals_brute(contigs, k, int(rng.choice([0, 0, 1, 7])))


def test_model_small_examples():
    iv = lambda contigs, k, slop=0: [as_pairs(r) for r in RM.all_intervals(contigs, [A.rep_kmer(k, slop)])[0][0]]
    assert iv([b"ACGGTTCA", b"GGACGGAA"], 4) == [[(0, 4)], [(2, 6)]]                 # a forward copy on another contig
    assert iv([b"AACCGTTA", b"GGAACGGT"], 5) == [[(1, 7)], [(2, 8)]]                 # reverse-complement copies: ACCGTT / AACGGT
    assert iv([b"TTACGTTT"], 4) == [[]]                                             # ACGT is a palindrome and occurs once
    assert iv([b"AAAAA"], 4) == [[(0, 5)]]                                          # k + 1 bases: both starts are repeated
    assert iv([b"AAAA"], 4) == [[]] and iv([b"AAAA", b"TTTT"], 4) == [[(0, 4)], [(0, 4)]]
    assert iv([b"GAAAAC", b"CCCAAAAGGG"], 4, 3) == [[(0, 6)], [(0, 10)]]            # slop clipped at both ends of a contig


# ---- the declarations

def test_header_and_library_agree():
    text = open(os.path.join(ROOT, "include", "vcfdist_repeats.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint\s+(vpr_\w+)\s*\(", code)
    assert sorted(names + ["vrp_write_repeat_bed"]) == sorted(api.REPEATS_EXPORTED) and len(names) == 7
    L = api.lib()
    for n in api.REPEATS_EXPORTED:
        assert hasattr(L, n), n
    fields = re.search(r"typedef struct vpr_repeat_stratum \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f for f, _ in A.VprRepeatStratum._fields_]
    defs = {n: int(v) for n, v in re.findall(r"#define (VPR_REP_\w+) (\d+)", text)}
    assert defs == {"VPR_REP_MIN_K": A.REP_MIN_K, "VPR_REP_MAX_K": A.REP_MAX_K, "VPR_REP_MAX_SPEC": A.REP_MAX_SPEC}
    assert len(RC.HAND_SPECS) == A.REP_MAX_SPEC
    assert "vrp_write_repeat_bed" in open(os.path.join(ROOT, "include", "vcfdist_report.h")).read()


def test_default_set():
    names, specs = api.repeats_default()
    assert names == ["rep_k16", "rep_k24", "rep_k32"] and [(s.k, s.slop) for s in specs] == [(16, 0), (24, 0), (32, 0)]


# ---- non-vacuity of the GPU tests' inputs

@pytest.mark.parametrize("k", RC.HAND_K)
def test_hand_cases_are_not_vacuous(k):
    cases = RC.hand_cases(k)
    iv = {n: [as_pairs(r) for r in RM.all_intervals(c, [A.rep_kmer(k)])[0][0]] for n, c in cases.items()}
    st = {n: RM.repeated(c, k)[1:] for n, c in cases.items()}
    lens = [len(c) for c in cases["lengths"]]
    assert lens[0] == k - 1 and lens[1] == k and lens[2] == 0
    assert iv["lengths"][0] == [] and iv["lengths"][1] == [(0, k)] and iv["lengths"][2] == [] and any(a <= k + 5 and b >= 2 * k + 5 for a, b in iv["lengths"][3])
    L = len(cases["n_invalidates_k"][0])
    assert st["n_invalidates_k"][0] == (L - k + 1) - k                        # the N takes exactly k starts
    assert any(a <= 9 and b >= 9 + k + 3 for a, b in iv["forward"][0]) and any(a <= k and b >= 2 * k + 3 for a, b in iv["forward"][1])
    assert any(a <= 9 and b >= 9 + k + 3 for a, b in iv["revcomp"][0]) and any(a <= k + 2 and b >= 2 * k + 5 for a, b in iv["revcomp"][1])
    if k >= 31:              # (at k = 4 and 5 random words repeat by chance; here a copy can at most be a base or two longer by chance)
        assert 3 * 4 <= st["forward"][1] <= 3 * 4 + 6 and 2 * 4 <= st["revcomp"][1] <= 2 * 4 + 4
        if k % 2 == 0:
            assert st["palindrome_once"][1] == 0 and iv["palindrome_once"] == [[]]
            assert st["palindrome_twice"][1] >= 2 and any(a <= k + 3 and b >= 2 * k + 3 for a, b in iv["palindrome_twice"][0])
        (a0, b0), (a1, b1) = iv["ends_on_last_base"][0][-1], iv["ends_on_last_base"][1][0]
        assert a0 <= k + 4 and b0 == 2 * k + 10 == len(cases["ends_on_last_base"][0]) and a1 == 0 and b1 >= k + 6
        rep = RM.repeated(cases["runs_one_apart"], k)[0][0]
        assert rep[5:8].all() and not rep[8] and rep[9:12].all()              # starts 0..2 and 4..6 of s, not 3
        assert len(iv["runs_one_apart"][0]) == 1 and iv["runs_one_apart"][0][0][0] <= 5 and iv["runs_one_apart"][0][0][1] >= 5 + 6 + k
    for n in ("poly_t", "poly_a"):
        assert iv[n] == [[(0, k + 8)]] and st[n] == (9, 9)
    assert iv["poly_t_and_a"] == [[(1, k + 1)], [(1, k + 1)]] and st["poly_t_and_a"][1] == 2
    assert st["none"][0] > 0 and st["none"][1] == 0 and iv["none"] == [[], []]


def test_seam_case_is_not_vacuous():
    bpw, _ = api.context_info()
    contigs, specs, plants = RC.seam_case(bpw)
    assert [len(c) for c in contigs] == list(RC.SEAM_LENGTHS) and 290_000 < sum(RC.SEAM_LENGTHS) < 310_000
    assert {p[1] for p in plants} == set(RC.SEAM_PLANT_LENGTHS) and min(RC.SEAM_PLANT_LENGTHS) == 20 and max(RC.SEAM_PLANT_LENGTHS) == 3000
    # every copy straddles a seam of the per-base kernels, half of them one of the run kernels
    assert all(a < (a + n // 2) // bpw * bpw + 1 <= a + n and (a + n // 2) % bpw == 0 for a, n in plants)
    assert sum((a + n // 2) % (4 * bpw) == 0 for a, n in plants) == len(plants) // 2
    rows, nv, nr = RM.all_intervals(contigs, specs)
    off = np.cumsum([0] + [len(c) for c in contigs])
    for k, sp in enumerate(specs):
        assert all(len(rows[k][c][0]) > 0 for c in range(3)), "an entry without an interval on a contig"
        assert all(not (len(rows[k][c][0]) == 1 and rows[k][c][0][0] == 0 and rows[k][c][1][0] == len(contigs[c])) for c in range(3))
        assert 0 < nr[k] < nv[k] < off[-1]
        # the word that ends contig 0 and begins contig 1: a tract to the last base, one from the first
        assert rows[k][0][1][-1] == len(contigs[0]) and rows[k][1][0][0] == 0
    # the copies of at least k bases lie inside an interval of the entry (k = 32, slop 0); the 20-base plant is none at k = 24
    def inside(k, a, n):
        c = int(np.searchsorted(off, a, "right")) - 1
        st, sp = rows[k][c]
        j = int(np.searchsorted(st, a - off[c], "right")) - 1
        return j >= 0 and sp[j] >= a - off[c] + n
    long_enough = [(a, n) for a, n in plants if n >= 32 and n != 1000]
    assert len(long_enough) >= 14 and all(inside(5, a, n) for a, n in long_enough)
    assert not any(inside(5, a, n) for a, n in plants if n == 1000)            # one copy holds an N: both are cut in two there
    assert not inside(3, *plants[0]) and inside(2, *plants[0])
    # the word cut by the start of contig 2: its halves end contig 1 and begin contig 2 (the k-mers across the cut do not exist)
    assert rows[5][1][1][-1] == len(contigs[1]) and rows[5][1][0][-1] <= len(contigs[1]) - 300 and rows[5][2][0][0] == 0
    assert nv[5] > 290_000                                     # the sort's keys span many blocks


def test_demo_fasta_is_not_vacuous():
    seq, sites = RC.demo_fasta()
    names, specs = api.repeats_default()
    rows, nv, nr = RM.all_intervals([seq], specs)
    half = RC.DEMO_WINDOW // 2
    for k in range(3):
        st, sp = rows[k][0]
        assert len(st) > 0
        for p in sites:                                        # every planted site lies inside an interval of every default stratum
            j = int(np.searchsorted(st, p, "right")) - 1
            assert j >= 0 and st[j] <= p - half + 1 and sp[j] >= p + half - 1, (k, p)
