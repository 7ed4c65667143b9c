"""The distance mode (-d) on the CPU: the model (tests/distance_model.cpp) on hand-derived alignments, the report writers
(vrp_write_distance / vrp_write_edits) against hand-written text and against the model's plain writers, the exported symbols,
and both command lines' argument checks.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import distance_helpers as DH  # noqa: E402

SUB, INS, DEL = 1, 2, 3
F_INS, F_DEL, F_MAT, F_SUB = 1, 2, 4, 8


def test_identical_strings():
    assert DH.job("ACGTACGTAC", "ACGTACGTAC", beg=100) == (0, [])


def test_one_snp_one_insertion_one_deletion():
    assert DH.job("ACGTACGT", "ACCTACGT", beg=100, sc=4, hap=1, minq=3, maxq=9) == (1, [(4, 1, 102, SUB, 1, 3, 9)])
    # query has an extra G after four A: an insertion at the position of the next reference base
    assert DH.job("AAAAGCCCC", "AAAACCCC", beg=10) == (1, [(0, 0, 14, INS, 1, 0, 62)])
    # truth has a G the query lacks: a deletion of that base
    assert DH.job("AAAACCCC", "AAAAGCCCC", beg=10) == (1, [(0, 0, 14, DEL, 1, 0, 62)])


def test_sub_run_gives_one_record_per_base():
    # three substitutions (9) beat a 3-base insertion plus deletion (10)
    d, rec = DH.job("AAAAAGGGAAAAA", "AAAAATTTAAAAA", beg=0)
    assert d == 3
    assert rec == [(0, 0, 5, SUB, 1, 0, 62), (0, 0, 6, SUB, 1, 0, 62), (0, 0, 7, SUB, 1, 0, 62)]


def test_run_open_at_the_end_is_counted_not_recorded():
    # The alignment runs on reversed strings, so the CIGAR's last step is the reversed alignment's first one, and the bounds
    # checks never let that be a gap (an INS from the start fails `diag + off >= 0`, a DEL from the start never closes into
    # SUB): a trailing gap becomes gap + SUB.  Truth with two extra bases at the end: DEL DEL SUB, the DEL run recorded
    # when the SUB run starts, the SUB run open at the end counted and never recorded.
    assert DH.steps("CCCC", "CCCCGG") == [F_MAT] * 3 + [F_DEL] * 2 + [F_SUB]
    assert DH.job("CCCC", "CCCCGG", beg=7) == (3, [(0, 0, 10, DEL, 2, 0, 62)])
    assert DH.steps("CCCCGG", "CCCC") == [F_MAT] * 3 + [F_INS] * 2 + [F_SUB]
    assert DH.job("CCCCGG", "CCCC", beg=7) == (3, [(0, 0, 10, INS, 2, 0, 62)])


def test_ored_ins_flag_walks_a_mismatch_as_a_match():
    # INS and DEL both close into one SUB cell; the backtrack follows INS, whose offset is smaller, and walks A/C as a "match"
    st = DH.steps("ACAC", "CCCAACA")
    assert st == [F_MAT, F_MAT, F_INS, F_DEL, F_DEL, F_DEL, F_DEL, F_SUB]
    assert "ACAC"[0] != "CCCAACA"[0]
    # counted: 1 INS + 4 DEL + 1 SUB (the mismatch walked as MAT counts 0); the trailing SUB run is never recorded
    assert DH.job("ACAC", "CCCAACA", beg=50) == (6, [(0, 0, 52, INS, 1, 0, 62), (0, 0, 52, DEL, 4, 0, 62)])


def _tiny_variants(quals):
    """one supercluster [0, 19] on a 20-base contig, three query SNPs on hap 1 with the given qualities, no truth variants"""
    from vcfdist_amd import _abi as A
    seq = np.frombuffer(b"ACGTACGTACGTACGTACGT", np.uint8).copy()
    pos = np.array([3, 8, 13], np.int32)
    pool = np.frombuffer(b"CCA", np.uint8).copy()            # ALT bases (reference T, A, C there)
    e32, e64, e8 = np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    return A.Variants(np.array([0, 20], np.int64), seq, np.zeros(1, np.int32), np.array([0], np.int32), np.array([19], np.int32),
                      [np.array([0, 3], np.int64)] + [np.array([0, 0], np.int64)] * 3,
                      [pos, e32, e32, e32], [np.full(3, SUB, np.uint8), e8, e8, e8],
                      [np.array(quals, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)],
                      [np.arange(3, dtype=np.int64), e64, e64, e64], [np.ones(3, np.int32), e32, e32, e32],
                      [np.arange(3, dtype=np.int64), e64, e64, e64], [np.ones(3, np.int32), e32, e32, e32],
                      [pool, np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint8)])


def test_threshold_sets_with_fractional_qualities():
    v = _tiny_variants([29.5, 30.2, 10.0])
    jobs, recs = DH.run(v, np.zeros(1, np.int32), np.zeros(1, np.uint8), max_qual=60)
    # hap 1: {int(q + 1)} = {30, 31, 11} u {62}; hap 2: {62}
    assert [tuple(j[:4]) for j in jobs] == [(0, 0, 0, 11), (0, 0, 11, 30), (0, 0, 30, 31), (0, 0, 31, 62), (0, 1, 0, 62)]
    # below 11 all three SNPs apply, from 11 the Q10 one is gone, from 30 the Q29.5 one, from 31 none
    assert [int(j[4]) for j in jobs] == [3, 2, 1, 0, 0]
    # the last SNP is at the region's 14th base of 20: every SUB run closes before the end, one record per SNP and job
    assert [tuple(r[2:]) for r in recs] == [(3, SUB, 1, 0, 11), (8, SUB, 1, 0, 11), (13, SUB, 1, 0, 11),
                                            (3, SUB, 1, 11, 30), (8, SUB, 1, 11, 30), (8, SUB, 1, 30, 31)]


# records of the hand-derived writer case: a SUB live at qualities [0, 3) and a 2-base INS live at [1, 4); min_qual 0, max_qual 2
HAND = [(0, 0, 10, SUB, 1, 0, 3), (0, 1, 20, INS, 2, 1, 4)]
HAND_DISTANCE = """MIN_QUAL\tSUB_DE\tINS_DE\tDEL_DE\tSUB_ED\tINS_ED\tDEL_ED\tDISTINCT_EDITS\tEDIT_DIST\tALN_SCORE\tALN_QSCORE
0\t1\t0\t0\t1\t0\t0\t1\t1\t3\t1.249387
1\t1\t1\t0\t1\t2\t0\t2\t3\t7\t0.000000
2\t1\t1\t0\t1\t2\t0\t2\t3\t7\t0.000000
3\t0\t1\t0\t0\t2\t0\t1\t2\t4\t0.000000
"""
# qscore(x / 0) = 0 (SNP NONE), qscore(0 / 0) = 0 (SNP BEST, every DEL row), qscore(0 / y) = 100 (INS / INDEL NONE);
# BEST = first quality minimising ED x DE: ALL 0 (1 x 1), SNP 3 (0 x 0), DEL 0 (all tie at 0).
# At verbosity 1 (the command lines') the reference skips INS and DEL before it writes a row (edit.cpp:212-217): 9 rows
HAND_SUMMARY = """VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE
ALL\tNONE\t0\t1\t1\t3.010300\t0.000000\t1.249387
ALL\tBEST\t0\t1\t1\t3.010300\t0.000000\t1.249387
ALL\tREF \t3\t2\t1\t0.000000\t0.000000\t0.000000
SNP\tNONE\t0\t1\t1\t0.000000\t0.000000\t0.000000
SNP\tBEST\t3\t0\t0\t0.000000\t0.000000\t0.000000
SNP\tREF \t3\t0\t0\t0.000000\t0.000000\t0.000000
INDEL\tNONE\t0\t0\t0\t100.000000\t100.000000\t0.000000
INDEL\tBEST\t0\t0\t0\t100.000000\t100.000000\t0.000000
INDEL\tREF \t3\t2\t1\t0.000000\t0.000000\t0.000000
"""
# verbosity 2: all five types
HAND_SUMMARY_V2 = """VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE
ALL\tNONE\t0\t1\t1\t3.010300\t0.000000\t1.249387
ALL\tBEST\t0\t1\t1\t3.010300\t0.000000\t1.249387
ALL\tREF \t3\t2\t1\t0.000000\t0.000000\t0.000000
SNP\tNONE\t0\t1\t1\t0.000000\t0.000000\t0.000000
SNP\tBEST\t3\t0\t0\t0.000000\t0.000000\t0.000000
SNP\tREF \t3\t0\t0\t0.000000\t0.000000\t0.000000
INS\tNONE\t0\t0\t0\t100.000000\t100.000000\t0.000000
INS\tBEST\t0\t0\t0\t100.000000\t100.000000\t0.000000
INS\tREF \t3\t2\t1\t0.000000\t0.000000\t0.000000
DEL\tNONE\t0\t0\t0\t0.000000\t0.000000\t0.000000
DEL\tBEST\t0\t0\t0\t0.000000\t0.000000\t0.000000
DEL\tREF \t3\t0\t0\t0.000000\t0.000000\t0.000000
INDEL\tNONE\t0\t0\t0\t100.000000\t100.000000\t0.000000
INDEL\tBEST\t0\t0\t0\t100.000000\t100.000000\t0.000000
INDEL\tREF \t3\t2\t1\t0.000000\t0.000000\t0.000000
"""
HAND_STDOUT = ("ALIGNMENT DISTANCE SUMMARY\n"
               "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE\n"
               "ALL\tNONE Q >= 0\t1               1               3.010300\t0.000000\t1.249387\n"
               "ALL\tBEST Q >= 0\t1               1               3.010300\t0.000000\t1.249387\n"
               "ALL\tREF  Q >= 3\t2               1               0.000000\t0.000000\t0.000000\n"
               "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\n"
               "SNP\tNONE Q >= 0\t1               1               0.000000\t0.000000\n"
               "SNP\tBEST Q >= 3\t0               0               0.000000\t0.000000\n"
               "SNP\tREF  Q >= 3\t0               0               0.000000\t0.000000\n"
               "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\n"
               "INDEL\tNONE Q >= 0\t0               0               100.000000\t100.000000\n"
               "INDEL\tBEST Q >= 0\t0               0               100.000000\t100.000000\n"
               "INDEL\tREF  Q >= 3\t2               1               0.000000\t0.000000\n")
HAND_EDITS = """CONTIG\tSTART\tHAP\tTYPE\tSIZE\tSUPERCLUSTER\tMIN_QUAL\tMAX_QUAL
chr1\t10\t0\tSNP\t1\t0\t0\t3
chr1\t20\t1\tINS\t2\t0\t1\t4
"""


def _read(p):
    with open(p) as f:
        return f.read()


def test_writers_against_hand_written_text(tmp_path):
    from vcfdist_amd import report as RP
    pre = str(tmp_path / "lib.")
    sets = [DH.sets_from_records("chr1", HAND)]
    text = RP.write_distance(pre, sets, 0, 2, 3, 2, 1)
    RP.write_edits(pre + "edits.tsv", sets)
    assert _read(pre + "distance.tsv") == HAND_DISTANCE
    assert _read(pre + "distance-summary.tsv") == HAND_SUMMARY
    assert _read(pre + "edits.tsv") == HAND_EDITS
    assert text == HAND_STDOUT
    assert len(HAND_SUMMARY.splitlines()) == 1 + 9
    v2 = str(tmp_path / "v2.")
    RP.write_distance(v2, sets, 0, 2, 3, 2, 1, verbosity=2)
    assert _read(v2 + "distance-summary.tsv") == HAND_SUMMARY_V2 and _read(v2 + "distance.tsv") == HAND_DISTANCE
    # the model's plain writers say the same
    mp = str(tmp_path / "model.")
    assert DH.write(mp, ["chr1"] * 2, HAND, 0, 2) == HAND_STDOUT
    for f in ("distance.tsv", "distance-summary.tsv", "edits.tsv"):
        assert _read(mp + f) == _read(pre + f), f
    # without files: the summary only
    nf = str(tmp_path / "none.")
    assert RP.write_distance(nf, sets, 0, 2, 3, 2, 1, write_files=False) == HAND_STDOUT
    assert not any(n.startswith("none.") for n in os.listdir(tmp_path))


def test_writers_difference_arrays_equal_the_rescan(tmp_path):
    """random record sets over two contigs: the library's difference arrays against the model's per-quality rescan, all verbosities"""
    from vcfdist_amd import report as RP
    rng = np.random.default_rng(5)
    for trial in range(6):
        n1, n2 = rng.integers(0, 60, 2)
        def recs(n):
            lo = rng.integers(-2, 25, n)
            return np.stack([rng.integers(0, 9, n), rng.integers(0, 2, n), rng.integers(0, 10**6, n), rng.integers(1, 4, n),
                             rng.integers(1, 40, n), lo, lo + rng.integers(0, 12, n)], 1).astype(np.int32)
        a, b = recs(n1), recs(n2)
        min_q, max_q = int(rng.integers(0, 4)), int(rng.integers(8, 22))
        x, o, e = (int(v) for v in rng.integers(1, 6, 3))
        for verb in (0, 1, 2):
            pre, mp = str(tmp_path / f"l{trial}{verb}."), str(tmp_path / f"m{trial}{verb}.")
            sets = [DH.sets_from_records("chrA", a), DH.sets_from_records("chrB", b)]
            got = RP.write_distance(pre, sets, min_q, max_q, x, o, e, verbosity=verb)
            RP.write_edits(pre + "edits.tsv", sets)
            want = DH.write(mp, ["chrA"] * len(a) + ["chrB"] * len(b), np.concatenate([a, b]), min_q, max_q, x, o, e, verbosity=verb)
            assert got == want
            for f in ("distance.tsv", "distance-summary.tsv", "edits.tsv"):
                assert _read(pre + f) == _read(mp + f), (trial, verb, f)


def test_distance_symbols_are_exported():
    from vcfdist_amd import api
    lib = api.lib()
    for name in ("vpr_distance", "vpr_distance_info", "vpr_distance_download", "vrp_write_distance", "vrp_write_edits"):
        assert hasattr(lib, name), name
    import re
    hdr = open(os.path.join(ROOT, "include", "vcfdist_distance.h")).read()
    declared = set(re.findall(r"\b(vpr_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(api.DIST_EXPORTED)
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("vpr_distance", "vpr_distance_download"):
        assert f" T {name}\n" in out, name


def _cli():
    return os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")


def test_command_lines_accept_and_check_the_distance_options(tmp_path):
    """-d -ex 4 -eo 3 -ee 2 get past argument parsing (the run then stops at the missing input file); -ex -1 is refused"""
    missing = str(tmp_path / "missing.vcf")
    ok = [missing, missing, missing, "-d", "-ex", "4", "-eo", "3", "-ee", "2"]
    r = subprocess.run([_cli()] + ok, capture_output=True, text=True)
    assert r.returncode != 0 and "unknown option" not in r.stderr and "penalty" not in r.stderr, r.stderr
    for bad, msg in ((["-ex", "-1"], "Must provide non-negative evaluation mismatch penalty"),
                     (["-eo", "x"], "Invalid eval gap-opening penalty provided"),
                     (["-ee", "-3"], "Must provide non-negative eval gap-extension penalty")):
        r = subprocess.run([_cli(), missing, missing, missing, "-d"] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, r.stderr
    py = [sys.executable, "-m", "vcfdist_amd"]
    r = subprocess.run(py + ok, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "unrecognized arguments" not in r.stderr and "penalty" not in r.stderr, r.stderr
    for bad, msg in ((["-ex", "-1"], "Must provide non-negative evaluation mismatch penalty"),
                     (["-eo", "x"], "Invalid eval gap-opening penalty provided")):
        r = subprocess.run(py + [missing, missing, missing, "-d"] + bad, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and msg in r.stderr, r.stderr
    # several ranks: refused with a clear message before anything is read
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run(py + ok, capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode != 0 and "one rank only" in r.stderr, r.stderr
