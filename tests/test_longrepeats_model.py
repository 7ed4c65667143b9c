"""The model of the long repeat strata (tests/longrepeats_model.py) against the numpy model of the repeat strata at k <= 32 (one
family of definitions), the tracts that the planted cases declare (tests/longrepeats_cases.py), the C ABI's declarations, and the
conditions under which the GPU tests do not pass vacuously."""
import os
import re

import numpy as np
import pytest

import longrepeats_cases as LC
import longrepeats_model as LM
import repeats_cases as RC
import repeats_model as RM
from vcfdist_amd import _abi as A
from vcfdist_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_pairs(row):
    return [(int(a), int(b)) for a, b in zip(*row)]


@pytest.mark.parametrize("k", [16, 32])
def test_model_equals_the_repeat_model_up_to_32(k):
    for name, contigs in RC.hand_cases(k).items():
        specs = [A.rep_kmer(k, 0), A.rep_kmer(k, 3)]
        got, want = LM.all_intervals(contigs, specs), RM.all_intervals(contigs, specs)
        assert not LM.same(got[0], want[0]), name
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), name


def test_model_small_examples():
    iv = lambda contigs, k, slop=0: [as_pairs(r) for r in LM.all_intervals(contigs, [A.rep_kmer(k, slop)])[0][0]]
    assert iv([b"ACGGTTCA", b"GGACGGAA"], 4) == [[(0, 4)], [(2, 6)]]
    assert iv([b"AACCGTTA", b"GGAACGGT"], 5) == [[(1, 7)], [(2, 8)]]                 # reverse-complement copies
    assert iv([b"TTACGTTT"], 4) == [[]]                                             # ACGT is a palindrome and occurs once
    assert iv([b"AAAAA"], 4) == [[(0, 5)]] and iv([b"AAAA"], 4) == [[]]


def test_schedule_and_hairpin_lengths():
    assert LC.levels(40) == [(32, 40)] and LC.levels(64) == [(32, 64)] and LC.levels(100) == [(32, 64), (64, 100)]
    assert LC.levels(250) == [(32, 64), (64, 128), (128, 250)] and LC.levels(256)[-1] == (128, 256) and LC.levels(65) == [(32, 64), (64, 65)]
    for k in LC.K:
        ds = LC.hairpin_deltas(k)
        last = LC.levels(k)[-1]
        assert last[1] - last[0] in ds                             # the last level's d (k + d is even: d and k - 2 a have k's parity)
        if k in (64, 128, 256):
            assert k // 2 in ds                                    # d == a
    assert 4 in LC.hairpin_deltas(100)        # the palindromic 32-mer in the middle of 104 bases is a half of the 64-mer at offset 36


@pytest.mark.parametrize("k", LC.K)
def test_cases_give_their_declared_tracts(k):
    cases = LC.cases(k)
    assert {"copies", "overlap", "seam", "lengths", "tiles"} <= set(cases) and any(n.startswith("hairpin_") for n in cases)
    assert ("palindrome_once" in cases) == (k % 2 == 0)
    assert [n for n in cases if n.startswith("seam_exact_")] == [f"seam_exact_{a}" for a in (32, 64, 128) if k >= 2 * a]
    for name, case in cases.items():
        contigs = case["contigs"]
        assert sum(len(c) for c in contigs) <= 26_000, name
        rows, n_valid, n_rep = LM.all_intervals(contigs, [A.rep_kmer(k, 0)])
        assert [as_pairs(r) for r in rows[0]] == case["tracts"], name
        # non-vacuous: a repeated start, except where nothing may be found
        assert (n_rep[0] == 0) == case["empty"] and n_valid[0] > 4000, name
    assert [len(c) for c in cases["lengths"]["contigs"]][:4] == [20, 0, k - 1, k] and len(cases["lengths"]["contigs"][5]) == 31
    assert cases["lengths"]["tracts"][3] == [(0, k)]
    (a, b), (c, d) = cases["tiles"]["tracts"][0][1:3]
    assert a < 4096 < b and c < 8192 < d
    assert len(LC.specs_of(k, "copies")) == A.LREP_MAX_SPEC and [(s.k, s.slop) for s in LC.specs_of(k, "seam")] == [(k, 0), (k, 5)]


def test_header_and_library_agree():
    text = open(os.path.join(ROOT, "include", "vcfdist_longrepeats.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint\s+(vpr_\w+)\s*\(", code)
    assert sorted(names + ["vrp_write_long_repeat_bed"]) == sorted(api.LONGREPEATS_EXPORTED) and len(names) == 6
    L = api.lib()
    for n in api.LONGREPEATS_EXPORTED:
        assert hasattr(L, n), n
    defs = {n: int(v) for n, v in re.findall(r"#define (VPR_LREP_\w+) (\d+)", text)}
    assert defs == {"VPR_LREP_MIN_K": A.LREP_MIN_K, "VPR_LREP_MAX_K": A.LREP_MAX_K, "VPR_LREP_MAX_SPEC": A.LREP_MAX_SPEC}
    assert A.LREP_MIN_K == A.REP_MAX_K + 1 and "GIAB" in text and "not a reproduction" in text.lower().replace("\n *", "")
    assert "vrp_write_long_repeat_bed" in open(os.path.join(ROOT, "include", "vcfdist_report.h")).read()
    from vcfdist_amd import report as RP
    assert "vrp_write_long_repeat_bed" in RP.EXPORTED


def test_default_set():
    names, specs = api.longrepeats_default()
    assert names == ["rep_k64", "rep_k100", "rep_k250"] and [(s.k, s.slop) for s in specs] == [(64, 0), (100, 0), (250, 0)]
    assert not set(names) & set(api.repeats_default()[0])


def test_command_line_inputs_are_not_vacuous():
    names, contigs = LC.cli_inputs()
    rows, n_valid, n_rep = LM.all_intervals(contigs, api.longrepeats_default()[1])
    assert all(len(rows[k][c][0]) > 0 for k in range(3) for c in range(2)) and (n_rep > 0).all()
    assert len(rows[0][0][0]) == 4 and len(rows[2][0][0]) == 2          # the 120-base copies are none at k = 250
