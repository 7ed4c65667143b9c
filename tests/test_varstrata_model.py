"""The brute-force model of the variant strata (tests/varstrata_model.py) on hand cases, the C ABI's declarations, the writer of
variant-strata.tsv, the command lines' parse-time behaviour, and the conditions the GPU tests' inputs (tests/varstrata_cases.py)
have to meet for those tests not to pass vacuously."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import strata_model as M
import varstrata_cases as VC
import varstrata_model as VM
from vcfdist_amd import _abi as A
from vcfdist_amd import api, report as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_NAMES = ["snp_ti", "snp_tv", "ins_1to5", "ins_6to15", "ins_16to49", "ins_ge50", "del_1to5", "del_6to15", "del_16to49", "del_ge50",
                 "hom", "het", "iso_50", "near_10"]


def test_header_and_library_agree():
    text = open(os.path.join(ROOT, "include", "vcfdist_varstrata.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint\s+(v(?:pr|rp)_\w+)\s*\(", code)
    assert sorted(names) == sorted(api.VARSTRATA_EXPORTED) and len(names) == 4
    L = api.lib()
    for n in names:
        assert hasattr(L, n), n
    fields = re.search(r"typedef struct vpr_variant_stratum \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f for f, _ in A.VprVariantStratum._fields_]
    kinds = [int(re.search(rf"#define VPR_VS_{k} (\d+)", text).group(1)) for k in ("SIZE", "TI", "TV", "HOM", "HET", "NEAR")]
    assert kinds == [A.VS_SIZE, A.VS_TI, A.VS_TV, A.VS_HOM, A.VS_HET, A.VS_NEAR]
    assert int(re.search(r"#define VPR_VS_MAX_SPEC (\d+)", text).group(1)) == A.VS_MAX_SPEC == 64


def test_default_set():
    names, specs = api.varstrata_default()
    assert names == DEFAULT_NAMES
    f = lambda s: tuple(getattr(s, n) for n, _ in A.VprVariantStratum._fields_)
    I, D = A.TYPE_INS, A.TYPE_DEL
    assert [f(s) for s in specs] == [
        (A.VS_TI, 0, 0, 0, 0, 0, 0), (A.VS_TV, 0, 0, 0, 0, 0, 0),
        (A.VS_SIZE, I, 1, 5, 0, 0, 0), (A.VS_SIZE, I, 6, 15, 0, 0, 0), (A.VS_SIZE, I, 16, 49, 0, 0, 0), (A.VS_SIZE, I, 50, 0, 0, 0, 0),
        (A.VS_SIZE, D, 1, 5, 0, 0, 0), (A.VS_SIZE, D, 6, 15, 0, 0, 0), (A.VS_SIZE, D, 16, 49, 0, 0, 0), (A.VS_SIZE, D, 50, 0, 0, 0, 0),
        (A.VS_HOM, 0, 0, 0, 0, 0, 0), (A.VS_HET, 0, 0, 0, 0, 0, 0), (A.VS_NEAR, 0, 0, 0, 50, 0, 0), (A.VS_NEAR, 0, 0, 0, 10, 1, -1)]


# ---- the model on the definitions

@pytest.fixture(scope="module")
def hand():
    v = VC.hand_case()
    names, specs = VC.hand_specs()
    bits = VM.members(v, specs)

    def strata(slot, ctg, pos, type=None):
        """names of the strata the variant is a member of"""
        i = VC.find(v, slot, ctg, pos, type)
        return {n for n, b in zip(names, bits[slot][:, i]) if b}
    return v, names, specs, bits, strata


def test_model_same_pos_and_copies(hand):
    v, names, specs, bits, strata = hand
    S, I, D = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL
    # a SNP and an insertion at one pos of one hap: neighbours at W 0, not copies, both het
    assert strata(0, 0, 10, S) == {"snp_ti", "het", "same_pos", "one_in_10", "near_10"}
    assert strata(0, 0, 10, I) == {"ins_1to5", "ins_2", "het", "same_pos", "one_in_10", "near_10"}
    # alleles equal except for the last ALT byte: no copy -- het, and each the other's neighbour
    assert strata(0, 0, 30) == strata(1, 0, 30) == {"ins_1to5", "het", "same_pos", "one_in_10", "near_10"}
    # a DEL copy (alt_len 0): hom, and alone at its pos (the two deletions at 60 are its neighbours at exactly W = 10); equal
    # lengths with other REF bytes are a copy too, another ref_len is not
    assert strata(0, 0, 50) == strata(1, 0, 50) == {"del_1to5", "del_any", "hom", "alone_at_pos", "two_in_10", "two_in_11", "near_10"}
    assert "hom" in strata(0, 0, 60) and "hom" in strata(1, 0, 60)
    assert "het" in strata(0, 0, 64) and "het" in strata(1, 0, 64) and "same_pos" in strata(0, 0, 64)
    # the 301-byte allele: hom on the truth, het on the query, whose alleles differ in the last byte alone
    assert strata(2, 1, 200) == strata(3, 1, 200) == {"ins_ge50", "ins_300", "hom", "alone_at_pos", "iso_50"}
    assert strata(0, 1, 200) == strata(1, 1, 200) == {"ins_ge50", "ins_300", "het", "same_pos", "one_in_10", "near_10"}


def test_model_windows(hand):
    v, names, specs, bits, strata = hand
    # 120 and 130 are exactly 10 apart, 130 and 141 are 11 apart
    assert strata(0, 0, 120) == {"snp_ti", "het", "alone_at_pos", "one_in_10", "near_10"}
    assert strata(1, 0, 130) == {"snp_ti", "het", "alone_at_pos", "one_in_10", "near_10", "two_in_11"}
    assert strata(0, 0, 141) == {"snp_tv", "het", "alone_at_pos"}
    # a hom pair: neither is its copy's neighbour, the insertion three bases on is; it counts the pair twice
    assert strata(0, 0, 200) == strata(1, 0, 200) == {"snp_tv", "hom", "alone_at_pos", "one_in_10", "near_10"}
    assert strata(1, 0, 203) == {"ins_1to5", "het", "alone_at_pos", "two_in_10", "two_in_11", "near_10"}


def test_model_bases_and_sizes(hand):
    v, names, specs, bits, strata = hand
    # an N on either side, lower case and an MNP are neither a transition nor a transversion
    for pos in (20, 25, 35, 40):
        assert not strata(2, 0, pos) & {"snp_ti", "snp_tv"}, pos
    ti_tv = {70: "snp_ti", 72: "snp_ti", 74: "snp_tv", 76: "snp_tv", 78: "snp_ti", 80: None, 82: "snp_tv", 84: "snp_tv"}
    for pos, want in ti_tv.items():
        assert strata(1, 0, pos) & {"snp_ti", "snp_tv"} == ({want} if want else set()), pos
    # the limits of every size bin
    bins = {1: "1to5", 5: "1to5", 6: "6to15", 15: "6to15", 16: "16to49", 49: "16to49", 50: "ge50", 51: "ge50"}
    for k, (n, b) in enumerate(bins.items()):
        assert strata(2, 1, 20 + 3 * k) & set(DEFAULT_NAMES[2:10]) == {"ins_" + b}, n
        assert strata(3, 1, 60 + 3 * k) & set(DEFAULT_NAMES[2:10]) == {"del_" + b}, n
        assert "del_any" in strata(3, 1, 60 + 3 * k) and "del_any" not in strata(2, 1, 20 + 3 * k)


def test_model_contig_ends(hand):
    v, names, specs, bits, strata = hand
    assert len(v.ctg_off) == 3 and v.n_vars(3) and not (M.var_contig(v, 3) == 0).any()          # truth hap 2 has nothing on contig 0
    # the same variant at 295 on contig 0 (truth hap 1) and on contig 1 (truth hap 2): no copy and no neighbour of each other
    assert strata(2, 0, 295) == strata(3, 1, 295) == {"snp_ti", "het", "alone_at_pos", "iso_50"}
    # a hom pair at the second base of contig 1, whose only neighbours are the indels further on
    assert strata(2, 1, 2) == strata(3, 1, 2) == {"snp_ti", "hom", "alone_at_pos"}
    # hom and het partition every slot; no variant is both a transition and a transversion
    for b in bits:
        assert (b[10] ^ b[11]).all() and not (b[0] & b[1]).any()


def test_words_of_appends_behind_old_bits():
    bits = np.array([[1, 0, 1], [0, 1, 1], [1, 1, 0]], bool)
    assert VM.words_of(bits).tolist() == [[5, 6, 3]]
    old = np.array([[(1 << 64) - 1, 0, 1 << 62]], np.uint64)
    w = VM.words_of(bits, 62, old)
    assert w.shape == (2, 3) and [hex(int(x)) for x in w[0]] == [hex((1 << 62) - 1 | 1 << 62), hex(1 << 63), hex(3 << 62)]
    assert w[1].tolist() == [1, 1, 0]


# ---- the writer

def test_writer_bytes(tmp_path):
    names, specs = api.varstrata_default()
    nq, nt = np.arange(14, dtype=np.int64) * 3, 10 ** 10 + np.arange(14, dtype=np.int64)
    pre = str(tmp_path) + "/w_"
    RP.write_variant_strata(pre, names + ["x"], specs + [A.vs_near(7, 2, 9)], list(nq) + [1], list(nt) + [2])
    want = ("STRATUM\tKIND\tTYPE\tMIN_LEN\tMAX_LEN\tWINDOW\tMIN_N\tMAX_N\tQUERY_VARS\tTRUTH_VARS\n"
            "snp_ti\tTI\t.\t.\t.\t.\t.\t.\t0\t10000000000\n"
            "snp_tv\tTV\t.\t.\t.\t.\t.\t.\t3\t10000000001\n"
            "ins_1to5\tSIZE\tINS\t1\t5\t.\t.\t.\t6\t10000000002\n"
            "ins_6to15\tSIZE\tINS\t6\t15\t.\t.\t.\t9\t10000000003\n"
            "ins_16to49\tSIZE\tINS\t16\t49\t.\t.\t.\t12\t10000000004\n"
            "ins_ge50\tSIZE\tINS\t50\t.\t.\t.\t.\t15\t10000000005\n"
            "del_1to5\tSIZE\tDEL\t1\t5\t.\t.\t.\t18\t10000000006\n"
            "del_6to15\tSIZE\tDEL\t6\t15\t.\t.\t.\t21\t10000000007\n"
            "del_16to49\tSIZE\tDEL\t16\t49\t.\t.\t.\t24\t10000000008\n"
            "del_ge50\tSIZE\tDEL\t50\t.\t.\t.\t.\t27\t10000000009\n"
            "hom\tHOM\t.\t.\t.\t.\t.\t.\t30\t10000000010\n"
            "het\tHET\t.\t.\t.\t.\t.\t.\t33\t10000000011\n"
            "iso_50\tNEAR\t.\t.\t.\t50\t0\t0\t36\t10000000012\n"
            "near_10\tNEAR\t.\t.\t.\t10\t1\t.\t39\t10000000013\n"
            "x\tNEAR\t.\t.\t.\t7\t2\t9\t1\t2\n")
    assert open(pre + "variant-strata.tsv", "rb").read() == want.encode()
    assert VM.tsv_text(names + ["x"], specs + [A.vs_near(7, 2, 9)], list(nq) + [1], list(nt) + [2]) == want
    with pytest.raises(RP.ReportError):
        RP.write_variant_strata(str(tmp_path / "no" / "such") + "/", names, specs, nq, nt)
    with pytest.raises(RP.ReportError):
        RP.write_variant_strata(pre, names, specs[:-1] + [A.VprVariantStratum(9, 0, 0, 0, 0, 0, 0)], nq, nt)


# ---- the command lines, up to where the inputs are read

def _lists(tmp_path):
    M.write_bed(tmp_path / "a.bed", [("chr1", 10, 20)])
    good, bad = tmp_path / "good.tsv", tmp_path / "bad.tsv"
    good.write_text("whole\ta.bed\n")
    bad.write_text("whole\ta.bed\nnear_10\ta.bed\n")
    return str(good), str(bad)


COMBOS = (["--stratify-variants"], ["--stratify-variants", "--stratify-context"], ["--stratify-variants", "--bootstrap", "4"],
          ["--stratify", "GOOD", "--stratify-variants"], ["--stratify-context", "--stratify", "GOOD", "--stratify-variants", "--bootstrap", "4", "-n"])


def test_cxx_command_line_parses_the_option(tmp_path):
    good, bad = _lists(tmp_path)
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    r = subprocess.run([cli] + missing + ["--stratify", bad, "--stratify-variants"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "duplicate stratum name 'near_10' (a variant stratum of --stratify-variants)" in r.stderr, r.stderr
    assert "no_query" not in r.stderr and r.stdout == ""                   # (ended before an input was opened)
    r = subprocess.run([cli] + missing + ["--stratify", bad], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "duplicate" not in r.stderr and "no_query" in r.stderr        # (the list alone is fine)
    for combo in COMBOS:
        r = subprocess.run([cli] + missing + [good if a == "GOOD" else a for a in combo], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "unknown option" not in r.stderr and "no_query" in r.stderr, (combo, r.stderr)


def test_python_command_line_parses_the_option(tmp_path):
    from vcfdist_amd.__main__ import main
    good, bad = _lists(tmp_path)
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    with pytest.raises(SystemExit) as e:
        main(missing + ["--stratify", bad, "--stratify-variants"])
    assert "duplicate stratum name 'near_10' (a variant stratum of --stratify-variants)" in str(e.value)
    for combo in COMBOS + (["--stratify", bad],):
        with pytest.raises(Exception) as e:                                    # (the first input does not exist)
            main(missing + [good if a == "GOOD" else bad if a == "BAD" else a for a in combo])
        assert not isinstance(e.value, SystemExit) or "no_query" in str(e.value), (combo, e.value)
        assert "no_query" in str(e.value), (combo, e.value)


# ---- non-vacuity of the GPU tests' inputs

def test_random_batch_is_not_vacuous():
    names, specs = api.varstrata_default()
    v = VC.random_variants()
    assert [v.n_vars(s) for s in range(4)] == [513, 257, 640, 300] and v.n_sc == 300 and len(v.ctg_off) == 3
    assert set(np.unique(v.sc_ctg)) == {0, 1} and (np.diff(v.sc_ctg) >= 0).all()
    bits = VM.members(v, specs)
    q, t = VM.member_counts(bits)
    assert (q > 0).all() and (t > 0).all(), (dict(zip(names, q)), dict(zip(names, t)))           # every default stratum, each callset
    lens = np.concatenate([v.var_alt_len[s] for s in range(4)])
    assert (lens == 1).any() and (lens >= 300).any()
    assert (np.diff(v.sc_beg)[np.diff(v.sc_ctg) == 0] < 250).any()                                # superclusters closer than 50 bases
    # runs of equal pos within a slot, and variants of both contigs in a slot
    assert any((np.diff(v.var_pos[s]) == 0).any() for s in range(4)) and len(set(M.var_contig(v, 0))) == 2
    e = VC.edge_variants()
    assert [e.n_vars(s) for s in range(4)] == [1, 0, 513, 0]
    eb = VM.members(e, specs)
    assert eb[0][11, 0] and not eb[0][10, 0] and eb[2][11].all() and eb[1].shape == (14, 0)      # nothing is hom without a partner


def test_counter_batches_are_not_vacuous():
    names, specs = api.varstrata_default()
    v = VC.synth().variants()
    bits = VM.members(v, specs)
    q, t = VM.member_counts(bits)
    for k in (0, 1, 2, 6, 10, 11, 12, 13):
        assert q[k] > 0 and t[k] > 0, names[k]
    s = VC.synth(snp_only=True).variants()
    assert all((s.var_type[h] == A.TYPE_SUB).all() for h in range(4))
    sb = VM.members(s, specs)
    assert all((b[0] | b[1]).all() for b in sb)                                                  # every SNP is a transition or a transversion
