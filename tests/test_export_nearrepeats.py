"""The near-repeat strata without a GPU: every symbol of include/vcfdist_nearrepeats.h and its writer is a defined dynamic symbol of
the built library, vpr_nearrepeat_name names the strata, and both command lines refuse a malformed --stratify-near-repeats with
the same ERROR line before an input is opened."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from vcfdist_amd import __main__ as CLI, _abi as A, api
from vcfdist_amd import report as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = "--stratify-near-repeats"
LIMITS = ": M must be 0 to 3 and K 8 (M + 1) to 32"
MALFORMED = [("32", "entry '32' is not K:M"), ("32:", "entry '32:' is not K:M"), (":1", "entry ':1' is not K:M"), ("", "entry '' is not K:M"),
             ("32:x", "entry '32:x' is not K:M"), ("k:1", "entry 'k:1' is not K:M"), ("32:-1", "entry '32:-1' is not K:M"),
             ("32:1:0", "entry '32:1:0' is not K:M"), ("32:1,", "entry '' is not K:M"), ("32:1,,24:1", "entry '' is not K:M"),
             ("32:1 ,24:1", "entry '32:1 ' is not K:M"), ("33:1", "entry '33:1'" + LIMITS), ("15:1", "entry '15:1'" + LIMITS),
             ("23:2", "entry '23:2'" + LIMITS), ("31:3", "entry '31:3'" + LIMITS), ("7:0", "entry '7:0'" + LIMITS), ("32:4", "entry '32:4'" + LIMITS),
             ("32:1,24:1,32:1", "duplicate entry '32:1'"), ("32:1,032:1", "duplicate entry '032:1'"),
             ("32:0,32:1,32:2,32:3,24:1", "more than 4 entries")]


def test_every_symbol_is_exported():
    hdr = open(os.path.join(ROOT, "include", "vcfdist_nearrepeats.h")).read()
    names = re.findall(r"^int (vpr_[a-z_0-9]+)\(", hdr, re.M)
    assert sorted(names + ["vrp_write_near_repeat_bed"]) == sorted(api.NEARREPEATS_EXPORTED) and len(names) == 6
    assert "vrp_write_near_repeat_bed" in open(os.path.join(ROOT, "include", "vcfdist_report.h")).read()
    assert "vrp_write_near_repeat_bed" in RP.EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vcfdist_amd", "lib", "libvcfdist_pr.so")], capture_output=True, text=True,
                         check=True).stdout
    defined = {l.split()[-1] for l in out.split("\n") if l}
    for name in api.NEARREPEATS_EXPORTED + ["k_near_keys", "k_near_probe"]:
        assert name in defined, name
    for name in api.NEARREPEATS_EXPORTED:
        assert hasattr(api.lib(), name)
    assert (A.NREP_MAX_M, A.NREP_MAX_K, A.NREP_MAX_SPEC) == tuple(int(re.search(rf"#define VPR_NREP_{w} (\d+)", hdr).group(1)) for w in ("MAX_M", "MAX_K", "MAX_SPEC"))
    assert re.search(r"typedef struct vpr_near_stratum \{ int32_t k, m, slop; \}", hdr) and C.sizeof(A.VprNearStratum) == 12
    for method in ("nearrepeat_intervals", "download_nearrepeat_intervals", "nearrepeat_stats", "nearrepeat_timing"):
        assert callable(getattr(api.PrecisionRecall, method))
    assert callable(RP.write_near_repeat_bed)


def test_names():
    assert api.nearrepeat_name(A.near_kmer(32, 1)) == "near_k32_m1" and api.nearrepeat_name(A.near_kmer(24, 2, 9)) == "near_k24_m2"
    L = api.lib()
    sp = A.near_kmer(16, 0)
    small = C.create_string_buffer(11)
    assert L.vpr_nearrepeat_name(C.byref(sp), small, 11) == -1 and L.vpr_nearrepeat_name(C.byref(sp), None, 11) == -1
    exact = C.create_string_buffer(12)
    assert L.vpr_nearrepeat_name(C.byref(sp), exact, 12) == 0 and exact.value == b"near_k16_m0"


def test_a_wellformed_argument_is_parsed():
    args = CLI.parse(["q.vcf", "t.vcf", "ref.fa", O, "32:1,24:2,16:0,032:3"])
    assert [(s.k, s.m, s.slop) for s in args.near] == [(32, 1, 0), (24, 2, 0), (16, 0, 0), (32, 3, 0)] and CLI.stratifying(args)
    args = CLI.parse(["q.vcf", "t.vcf", "ref.fa"])
    assert args.near == [] and not CLI.stratifying(args)
    CLI.parse(["q.vcf", "t.vcf", "ref.fa", O, "32:1", "--classify-errors", "--cut-classes"])       # (a --stratify* option for --cut-classes)


@pytest.mark.parametrize("value,what", MALFORMED)
def test_both_drivers_refuse_a_malformed_argument_alike(tmp_path, value, what):
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa")]
    want = f"ERROR: {O}: {what}"
    with pytest.raises(SystemExit) as e:
        CLI.main(missing + [O, value])
    assert str(e.value) == want
    r = subprocess.run([os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")] + missing + [O, value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr == want + "\n" and r.stdout == ""


def test_a_near_repeat_name_in_the_list_is_refused(tmp_path):
    (tmp_path / "a.bed").write_text("chr1\t10\t20\n")
    lst = tmp_path / "list.tsv"
    lst.write_text("whole\ta.bed\nnear_k24_m2\ta.bed\n")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa")]
    want = f"ERROR: strata list '{lst}': duplicate stratum name 'near_k24_m2' (a near repeat stratum of {O})"
    with pytest.raises(SystemExit) as e:
        CLI.main(missing + ["--stratify", str(lst), O, "32:1,24:2"])
    assert str(e.value) == want
    r = subprocess.run([os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")] + missing + ["--stratify", str(lst), O, "32:1,24:2"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr == want + "\n"
    with pytest.raises(Exception) as e:             # (with other entries the list is fine: the first input does not exist)
        CLI.main(missing + ["--stratify", str(lst), O, "32:1"])
    assert "no_query" in str(e.value)
