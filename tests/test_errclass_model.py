"""The brute-force model of the error classes (tests/errclass_model.py) on the hand cases evaluated by the CPU oracle, the C ABI's
declarations, the writer of error-classes*.tsv, the command lines' parse-time behaviour, and the conditions the GPU tests' inputs
(tests/errclass_cases.py) have to meet for those tests not to pass vacuously."""
import os
import re
import subprocess

import numpy as np
import pytest

import errclass_cases as EC
import errclass_model as EM
import oracle_lib as O
from vcfdist_amd import _abi as A
from vcfdist_amd import api, report as RP, shard, summary as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def evaluated(v, sv_threshold=50):
    """a batch through the CPU oracle: results, phase-block phasing (one phase set) and the variant classes"""
    batch = O.generate(v)
    res = O.run(batch)
    pb, _, _ = S.phase(res.sc_phase, np.zeros(v.n_sc, np.int32), L=O.lib(), prefix="vso")
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold) for s in range(4)]
    return batch, res, pb, cls


def check_invariant(v, batch, res, pb, cls, cl, min_qual=0, max_qual=60):
    """for every type and threshold the query's classes sum to the counters' query FP, the truth's to their truth FN"""
    cnt = EM.counts(v, res, pb, cl, cls, min_qual, max_qual)
    plain = O.oracle_pr_counts(O.lib(), batch.var_off, res, cls, pb, min_qual, max_qual)
    assert np.array_equal(cnt[0].sum(1), plain[0, :, A.ERRTYPE_FP]) and np.array_equal(cnt[1].sum(1), plain[1, :, A.ERRTYPE_FN])
    assert not cnt[0, :, A.EC_LOWQ].any() and np.array_equal(cnt[:, 3], cnt[:, :3].sum(1))
    return cnt, plain


def test_header_and_library_agree():
    text = open(os.path.join(ROOT, "include", "vcfdist_errclass.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b(v(?:pr|rp)_\w+)\s*\(", code)
    assert sorted(names) == sorted(api.ERRCLASS_EXPORTED) and len(names) == 6
    L = api.lib()
    for n in names:
        assert hasattr(L, n), n
    codes = [int(re.search(rf"#define VPR_EC_{k} (\d+)", text).group(1)) for k in ("GT", "SYNC", "PHASE", "SITE", "NEAR", "ALONE", "LOWQ", "CLASSES", "NONE")]
    assert codes == [A.EC_GT, A.EC_SYNC, A.EC_PHASE, A.EC_SITE, A.EC_NEAR, A.EC_ALONE, A.EC_LOWQ, A.EC_CLASSES, A.EC_NONE] == [0, 1, 2, 3, 4, 5, 6, 7, 255]
    assert int(re.search(r"#define VPR_EC_DEFAULT_WINDOW (\d+)", text).group(1)) == A.EC_DEFAULT_WINDOW == 50
    assert api.errclass_names() == EM.NAMES == ["gt", "sync", "phase", "site", "near", "alone", "lowq"]
    # these are this project's definitions, and both the header and the README say so in bold
    assert "NOT a reproduction of\n * hap.py**" in text
    assert re.search(r"\*\*[^*]*not a\s+reproduction of hap\.py[^*]*\*\*", open(os.path.join(ROOT, "README.md")).read(), re.S)


# ---- the model on the definitions

@pytest.fixture(scope="module")
def hand():
    v, cases = EC.hand_case()
    batch, res, pb, cls = evaluated(v)
    return dict(v=v, cases=cases, batch=batch, res=res, pb=pb, cls=cls)


def test_hand_cases_literally(hand):
    v, cases, res, pb = hand["v"], hand["cases"], hand["res"], hand["pb"]
    # the phasings the cases are built for: ORIG, SWAP, and NONE where either costs the same
    ph = {n: int(res.sc_phase[k]) for n, k in cases.items()}
    assert ph["phase_orig"] == ph["long_tail"] == ph["long_copy"] == A.PHASE_ORIG and ph["phase_swap"] == A.PHASE_SWAP
    assert ph["gt_query"] == ph["gt_truth"] == ph["site"] == A.PHASE_NONE
    for window in EC.WINDOWS:
        cl = EM.classes(v, res, pb, window)
        for name, slot, k, want in EC.expect(window):
            assert cl[slot][EC.index_of(v, cases, name, slot, k)] == want, (window, name, slot, k)
        # zygosity: one copy matches, the other is the error (which one is the phasing's choice), in either callset
        for name, slots in (("gt_query", (0, 1)), ("gt_truth", (2, 3))):
            got = sorted(int(cl[s][EC.index_of(v, cases, name, s)]) for s in slots)
            assert got == [A.EC_GT, A.EC_LOWQ if slots[0] else A.EC_NONE], (name, got)
    # window 2^31 - 1: nothing wraps; whatever has a neighbour in its supercluster is near
    cl = EM.classes(v, res, pb, 2 ** 31 - 1)
    assert cl[0][EC.index_of(v, cases, "dist_51", 0)] == A.EC_NEAR and cl[0][EC.index_of(v, cases, "lone_query", 0)] == A.EC_ALONE


@pytest.mark.parametrize("pb_kind", ["null", "zeros", "ones"])
def test_hand_cases_under_either_phase_block_phasing(hand, pb_kind):
    """the superclusters left NONE follow pb_phase: the classes of the symmetric cases do not depend on it, gt moves to the other copy"""
    v, cases, res = hand["v"], hand["cases"], hand["res"]
    pb = None if pb_kind == "null" else np.full(v.n_sc, pb_kind == "ones", np.int32)
    cl = EM.classes(v, res, pb, 50)
    for name, slot, k, want in EC.expect(50):
        assert cl[slot][EC.index_of(v, cases, name, slot, k)] == want, (name, slot, k)
    w = int(pb_kind == "ones")
    # query hom / truth het on truth 1: the query haplotype aligned to the empty truth 2 holds the error
    assert cl[1 ^ w][EC.index_of(v, cases, "gt_query", 1 ^ w)] == A.EC_GT and cl[w][EC.index_of(v, cases, "gt_query", w)] == A.EC_NONE
    assert cl[3][EC.index_of(v, cases, "gt_truth", 3)] == A.EC_GT if w == 0 else cl[2][EC.index_of(v, cases, "gt_truth", 2)] == A.EC_GT


def test_every_class_has_members_and_the_invariant_holds(hand):
    v, batch, res, pb, cls = hand["v"], hand["batch"], hand["res"], hand["pb"], hand["cls"]
    cl = EM.classes(v, res, pb, 50)
    assert EC.populated(cl) == (list(range(6)), list(range(7)))                    # six in the query, seven in the truth
    assert all((c[:0] == c[:0]).all() and set(np.unique(c)) <= set(range(7)) | {A.EC_NONE} for c in cl)
    for mn, mx in ((0, 60), (15, 40), (30, 30), (0, 4)):
        cnt, plain = check_invariant(v, batch, res, pb, cls, cl, mn, mx)
        assert plain[0, 3, A.ERRTYPE_FP].any() and plain[1, 3, A.ERRTYPE_FN].any()
    # the quality cases: a query FP below min_qual counts at no threshold, a matched truth variant of quality 10 is FN above 10
    cnt, _ = check_invariant(v, batch, res, pb, cls, cl, 15, 40)
    full, _ = check_invariant(v, batch, res, pb, cls, cl, 0, 60)
    assert full[0, 0, A.EC_ALONE, 5] - full[0, 0, A.EC_ALONE, 6] == 2 and cnt[0, 0, A.EC_ALONE, 0] == full[0, 0, A.EC_ALONE, 15]
    assert full[1, 0, A.EC_LOWQ, 10] + 2 == full[1, 0, A.EC_LOWQ, 11] and cnt[1, 0, A.EC_LOWQ, 0] >= 2 and full[1, 0, A.EC_LOWQ, 0] == 0
    assert (np.diff(full[1, :, :6], axis=-1) == 0).all()                            # a truth FN counts at every threshold


# ---- non-vacuity of the GPU tests' inputs

def test_random_and_edge_batches_are_not_vacuous():
    v = EC.random_variants()
    assert [v.n_vars(s) for s in range(4)] == [513, 257, 640, 300] and v.n_sc == 300
    batch, res, pb, cls = evaluated(v, sv_threshold=6)
    assert (res.sc_phase == A.PHASE_ORIG).any() and (res.sc_phase == A.PHASE_SWAP).any() and (res.sc_phase == A.PHASE_NONE).any()
    cl = EM.classes(v, res, pb, 50)
    assert EC.populated(cl) == (EC.RANDOM_POPULATED_QUERY, EC.RANDOM_POPULATED_TRUTH)
    cnt, plain = check_invariant(v, batch, res, pb, cls, cl)
    assert all(plain[:, t].any() for t in range(3))                                 # SNP, INDEL and SV rows
    assert any((np.diff(v.var_pos[s]) == 0).any() for s in range(4))                # runs of equal pos within a slot
    e = EC.edge_variants()
    assert [e.n_vars(s) for s in range(4)] == [1, 0, 513, 0]
    batch, res, pb, cls = evaluated(e)
    cl = EM.classes(e, res, pb, 50)
    assert (cl[2] == A.EC_ALONE).sum() > 400 and cl[1].shape == (0,)
    check_invariant(e, batch, res, pb, cls, cl)


def test_demo_classes():
    """the classes the demo callsets populate: the command-line test may assert non-vacuity for these only"""
    import demo_pipeline as D
    rows, det = D.run(product=False)
    v, cls = EC.demo_variants(det)
    cl = EM.classes(v, det["res"], det["pb"], 50)
    assert EC.populated(cl) == (EC.DEMO_POPULATED_QUERY, EC.DEMO_POPULATED_TRUTH)
    cnt, plain = check_invariant(v, det["batch"], det["res"], det["pb"], cls, cl, D.G["min_qual"], D.G["max_qual"])
    assert np.array_equal(plain, det["counts"])


# ---- the share of a rank

def test_subset_variants_keeps_the_classes(hand):
    """everything is local to the supercluster: a rank's share, in any order, gives its variants the classes of the whole"""
    v, res, pb = hand["v"], hand["res"], hand["pb"]
    whole = EM.classes(v, res, pb, 50)
    idx = np.array([16, 3, 2, 9, 0, 14], np.int64)
    part = shard.subset_variants(v, idx)
    assert part.n_sc == 6 and part.allele_pool[0] is v.allele_pool[0]
    cut = lambda cols, s: shard.subset_per_variant(cols, v.var_off[s], idx)
    import types
    res_part = types.SimpleNamespace(sc_phase=res.sc_phase[idx], errtype=[[cut(res.errtype[s][w], s) for w in range(2)] for s in range(4)],
                                     callq=[[cut(res.callq[s][w], s) for w in range(2)] for s in range(4)])
    got = EM.classes(part, res_part, pb[idx], 50)
    for s in range(4):
        assert np.array_equal(got[s], cut(whole[s], s)) and len(got[s]) == part.n_vars(s)


# ---- the writer

def test_writer_equals_the_model(hand, tmp_path):
    v, batch, res, pb, cls = hand["v"], hand["batch"], hand["res"], hand["pb"], hand["cls"]
    cl = EM.classes(v, res, pb, 50)
    for mn, mx in ((0, 60), (15, 40)):
        cnt, plain = check_invariant(v, batch, res, pb, cls, cl, mn, mx)
        pre = str(tmp_path / f"{mn}_{mx}_")
        RP.write_error_classes(pre, cnt, plain, mn, mx)
        want_all, want_sum = EM.tsv_text(cnt, plain, mn, mx)
        assert open(pre + "error-classes.tsv").read() == want_all and open(pre + "error-classes-summary.tsv").read() == want_sum
        head = want_sum.split("\n")[0].split("\t")
        assert head[:3] == ["VAR_TYPE", "THRESHOLD", "MIN_QUAL"] and head[3:] == EM.COLUMNS and len(EM.COLUMNS) == 15
        assert len(want_all.split("\n")) == 4 * (mx - mn + 1) + 2 and len(want_sum.split("\n")) == 10
    assert "ALL\tNONE\t0\t24\t" in EM.tsv_text(*check_invariant(v, batch, res, pb, cls, cl))[1]
    with pytest.raises(RP.ReportError):
        RP.write_error_classes(str(tmp_path / "no" / "such") + "/", cnt, plain, 15, 40)
    with pytest.raises(RP.ReportError):
        RP.write_error_classes(pre, cnt, plain, 0, 60)                              # counts of another number of thresholds


# ---- the command lines, up to where the inputs are read

BAD_OPTIONS = ((["--error-window", "10"], "--error-window needs --classify-errors"), (["--classify-errors", "--error-window", "-1"], "error window"),
               (["--classify-errors", "--error-window", "x"], "error window"))
GOOD_OPTIONS = (["--classify-errors"], ["--classify-errors", "--error-window", "0"], ["--error-window", "2147483647", "--classify-errors", "-n"],
                ["--classify-errors", "--stratify-variants", "--bootstrap", "4"])


def test_cxx_command_line_parses_the_options(tmp_path):
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    for opts, text in BAD_OPTIONS:
        r = subprocess.run([cli] + missing + opts, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and text in r.stderr and "no_query" not in r.stderr and r.stdout == "", (opts, r.stderr)
    for opts in GOOD_OPTIONS:
        r = subprocess.run([cli] + missing + opts, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "unknown option" not in r.stderr and "no_query" in r.stderr, (opts, r.stderr)


def test_python_command_line_parses_the_options(tmp_path, capsys):
    from vcfdist_amd.__main__ import main
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa"), "-p", str(tmp_path) + "/"]
    for opts, text in BAD_OPTIONS:
        with pytest.raises(SystemExit) as e:
            main(missing + opts)
        assert text in str(e.value) + capsys.readouterr().err, opts
    for opts in GOOD_OPTIONS:
        with pytest.raises(Exception) as e:                                        # (the first input does not exist)
            main(missing + opts)
        assert "no_query" in str(e.value), (opts, e.value)
