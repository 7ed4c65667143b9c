"""The realignment's CPU model (tests/realign_model.py) on hand-derived cases at the default penalties 5 / 6 / 2, and the VCF writer
vrp_write_vcf (include/vcfdist_report.h) against hand-written text.  No GPU."""
import datetime
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import realign_model as RM  # noqa: E402

S, I, D = RM.SUB, RM.INS, RM.DEL


def hap(vs):
    """[(pos, type, ref, alt, qual, ps)] -> column dict"""
    recs = [dict(pos=p, rlen=len(r), type=t, ref=r, alt=a, var_qual=np.float32(q), gt_qual=np.float32(30), phase_set=ps, orig_gt=4)
            for p, t, r, a, q, ps in vs]
    return RM.columns(recs)


def run(seq, vs, cl=None, **kw):
    h = hap(vs)
    var_beg = cl if cl is not None else [0, len(vs)]
    recs, st = RM.realign(seq, h, var_beg, **kw)
    return [(r["pos"], r["type"], r["ref"], r["alt"]) for r in recs], recs, st


def test_cancelling_del_and_ins_realign_to_nothing():
    # CATATATG: DEL of the first AT, INS of AT two bases later -> the haplotype is the reference
    got, _, st = run("CATATATG", [(1, D, "AT", "", 30, 0), (5, I, "", "AT", 30, 0)])
    assert got == [] and st.tolist() == [0]


def test_four_subs_become_ins_and_del():
    # GACGTG read on the reference GCGTAG as four SUBs (20) realigns to INS A + DEL A (2 x (6 + 2) = 16)
    vs = [(1, S, "C", "A", 30, 0), (2, S, "G", "C", 30, 0), (3, S, "T", "G", 30, 0), (4, S, "A", "T", 30, 0)]
    got, _, _ = run("GCGTAG", vs)
    assert got == [(1, I, "", "A"), (4, D, "A", "")]
    import distance_helpers as DH
    steps = DH.steps("GACGTG", "GCGTAG", 5, 6, 2)
    opens = sum(1 for k, s in enumerate(steps) if s in (RM.F_INS, RM.F_DEL) and (k == 0 or steps[k - 1] != s))
    cost = 5 * steps.count(RM.F_SUB) + 6 * opens + 2 * (steps.count(RM.F_INS) + steps.count(RM.F_DEL))
    assert cost == 16


def test_ins_at_the_right_end_of_a_homopolymer_moves_left():
    got, _, _ = run("GAAAAC", [(5, I, "", "A", 30, 0)])
    assert got == [(1, I, "", "A")]


def test_quality_is_the_truncated_minimum_and_ps_the_first_nonzero():
    vs = [(2, S, "G", "T", 37.9, 0), (4, S, "T", "A", 12.7, 44), (6, S, "C", "A", 50.0, 99)]
    got, recs, _ = run("ACGGTACGT", vs)
    assert [(r[0], r[1]) for r in got] == [(2, S), (4, S), (6, S)]
    assert {float(r["var_qual"]) for r in recs} == {12.0} and {r["phase_set"] for r in recs} == {44}
    assert {float(r["gt_qual"]) for r in recs} == {60.0} and {r["orig_gt"] for r in recs} == {RM.GT_REF_REF}
    _, recs, _ = run("ACGGTACGT", vs, max_qual=10)
    assert {float(r["var_qual"]) for r in recs} == {10.0}


def test_second_pass_swaps_records_but_not_phase_sets():
    recs = [dict(pos=3, rlen=1, type=S, ref="A", alt="C", var_qual=np.float32(1), gt_qual=np.float32(2), phase_set=7, orig_gt=3),
            dict(pos=3, rlen=0, type=I, ref="", alt="GG", var_qual=np.float32(5), gt_qual=np.float32(6), phase_set=9, orig_gt=5)]
    RM.left_shift(recs, "TTTTTTTT")
    assert [(r["pos"], r["type"], r["ref"], r["alt"], float(r["var_qual"]), r["phase_set"], r["orig_gt"]) for r in recs] == \
        [(3, I, "", "GG", 5.0, 7, 5), (3, S, "A", "C", 1.0, 9, 3)]


def test_a_cluster_at_position_zero_keeps_its_variants():
    got, recs, st = run("ACGTACGT", [(0, S, "A", "G", 20, 0), (1, S, "C", "T", 20, 0)])
    assert st.tolist() == [RM.ST_EDGE] and got == [(0, S, "A", "G"), (1, S, "C", "T")]
    assert {r["orig_gt"] for r in recs} == {4} and {float(r["var_qual"]) for r in recs} == {20.0}


def test_overlapping_variants_are_an_error_and_keep_their_variants():
    vs = [(2, D, "GT", "", 20, 0), (3, S, "T", "A", 20, 0), (6, S, "G", "T", 20, 0)]
    got, _, st = run("ACGTACGTAC", vs)
    assert st.tolist() == [RM.ST_ERROR] and got == [(2, D, "GT", ""), (3, S, "T", "A"), (6, S, "G", "T")]


def test_region_past_the_contig_end_is_clamped():
    # a DEL of the last base: the region ends one past the contig
    seq = "ACGTAC"
    got, recs, st = run(seq, [(5, D, "C", "", 20, 0)])
    assert st.tolist() == [0] and got and all(4 <= r["pos"] and r["pos"] + r["rlen"] <= len(seq) for r in recs)
    # the realigned records spell the same haplotype over the clamped region [4, 6): "A"
    hapl, pos = "", 4
    for r in recs:
        hapl += seq[pos:r["pos"]] + r["alt"]
        pos = r["pos"] + r["rlen"]
    assert hapl + seq[pos:] == "A"


# ---- the writer

def _lib():
    from vcfdist_amd import api
    return api.lib()


def test_write_vcf_against_hand_written_text(tmp_path):
    _lib()
    from vcfdist_amd import report as RP
    seq = np.frombuffer(b"GATTACAGATTACA", np.uint8)
    recs1 = [dict(pos=2, rlen=1, type=S, ref="T", alt="C", var_qual=np.float32(30), gt_qual=np.float32(60), phase_set=0, orig_gt=2),
             dict(pos=6, rlen=0, type=I, ref="", alt="TT", var_qual=np.float32(12.5), gt_qual=np.float32(60), phase_set=0, orig_gt=2),
             dict(pos=9, rlen=2, type=D, ref="TT", alt="", var_qual=np.float32(7), gt_qual=np.float32(60), phase_set=0, orig_gt=2)]
    recs2 = [dict(pos=2, rlen=1, type=S, ref="T", alt="C", var_qual=np.float32(30), gt_qual=np.float32(60), phase_set=0, orig_gt=2),
             dict(pos=6, rlen=0, type=I, ref="", alt="G", var_qual=np.float32(3), gt_qual=np.float32(60), phase_set=0, orig_gt=2)]
    mono = [dict(pos=4, rlen=1, type=S, ref="A", alt="G", var_qual=np.float32(1), gt_qual=np.float32(60), phase_set=0, orig_gt=2)]
    cs = dict(contigs=["chr1", "chrY"], lengths=[14, 14], ploidy=[2, 1], sample="HG002",
              vars=[[RM.columns(recs1), RM.columns(recs2)], [RM.columns(mono), RM.columns([])]])
    fasta = {"chr1": seq, "chrY": seq}
    p = str(tmp_path / "t.vcf")
    RP.write_vcf(p, cs, fasta)
    today = datetime.date.today().strftime("%Y%m%d")
    want = ("##fileformat=VCFv4.2\n"
            f"##fileDate={today}\n"
            "##contig=<ID=chr1,length=14,ploidy=2>\n"
            "##contig=<ID=chrY,length=14,ploidy=1>\n"
            '##FILTER=<ID=PASS,Description="All filters passed">\n'
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tHG002\n"
            "chr1\t3\t.\tT\tC\t30.000000\tPASS\t.\tGT\t1|1\n"
            "chr1\t6\t.\tC\tCTT\t12.500000\tPASS\t.\tGT\t1|0\n"
            "chr1\t6\t.\tC\tCG\t3.000000\tPASS\t.\tGT\t0|1\n"
            "chr1\t9\t.\tATT\tA\t7.000000\tPASS\t.\tGT\t1|0\n"
            "chrY\t5\t.\tA\tG\t1.000000\tPASS\t.\tGT\t1\n")
    got = open(p).read()
    if got.split("\n")[1] != f"##fileDate={today}":        # (the day may have turned between the two reads of the clock)
        today = datetime.date.today().strftime("%Y%m%d")
        want = want.replace(want.split("\n")[1], f"##fileDate={today}")
    assert got == want
    hap_recs = [[recs1, recs2], [mono, []]]
    assert RM.write_vcf([("chr1", 14, 2, hap_recs[0]), ("chrY", 14, 1, hap_recs[1])], "HG002", fasta, today) == want


def test_realign_symbols_are_exported():
    from vcfdist_amd import api
    lib = _lib()
    import re
    hdr = open(os.path.join(ROOT, "include", "vcfdist_realign.h")).read()
    assert set(re.findall(r"\b(vrl_[a-z_0-9]+)\s*\(", hdr)) == set(api.RL_EXPORTED)
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    for name in api.RL_EXPORTED + ["vrp_write_vcf"]:
        assert hasattr(lib, name) and f" T {name}\n" in out, name


def _cli():
    return os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")


def test_command_lines_accept_the_realign_options(tmp_path):
    """-rq -rt -ro get past argument parsing (the run then stops at the missing input file); -x 0 with realignment is refused"""
    missing = str(tmp_path / "missing.vcf")
    for cmd, unknown in (([_cli()], "unknown option"), ([sys.executable, "-m", "vcfdist_amd"], "unrecognized arguments")):
        r = subprocess.run(cmd + [missing, missing, missing, "-rq", "-rt", "-ro"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and unknown not in r.stderr, r.stderr
        r = subprocess.run(cmd + [missing, missing, missing, "-rq", "-x", "0"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and "at least 1" in r.stderr, r.stderr
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run([sys.executable, "-m", "vcfdist_amd", missing, missing, missing, "-rq"], capture_output=True, text=True, cwd=ROOT,
                       env=env)
    assert r.returncode != 0 and "one rank only" in r.stderr, r.stderr
