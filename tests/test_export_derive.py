"""The derived strata without a GPU: every symbol of include/vcfdist_derive.h is a defined dynamic symbol of the built library,
k_derive_mask too, the constants agree between the header and _abi.py, and both command lines refuse every malformed
--stratify-derive / --stratify-cross with the same ERROR line, stdout empty, before an input is opened."""
import os
import re
import subprocess

import pytest

import derive_cases as DC
from vcfdist_amd import __main__ as CLI, _abi as A, api
from vcfdist_amd import report as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_CLI = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
D, X = "--stratify-derive", "--stratify-cross"
OTHERS = ["--stratify-context", "--stratify-variants"]          # the names of tests/derive_cases.py


def test_every_symbol_is_exported():
    hdr = open(os.path.join(ROOT, "include", "vcfdist_derive.h")).read()
    names = re.findall(r"^(?:int|const char \*)\s*(v[pr][rp]_[a-z_0-9]+)\(", hdr, re.M)
    assert sorted(names) == sorted(api.DERIVE_EXPORTED) and len(names) == 6
    assert "vrp_write_derived_strata" in RP.EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vcfdist_amd", "lib", "libvcfdist_pr.so")], capture_output=True, text=True,
                         check=True).stdout
    defined = {l.split()[-1] for l in out.split("\n") if l}
    for name in api.DERIVE_EXPORTED + ["k_derive_mask"]:
        assert name in defined, name
    for name in api.DERIVE_EXPORTED:
        assert hasattr(api.lib(), name)
    const = lambda w: int(re.search(rf"#define VPR_DV_{w} \(?(-?\d+)\)?", hdr).group(1))
    assert (A.DV_AND, A.DV_OR, A.DV_NOT) == (const("AND"), const("OR"), const("NOT")) == (-1, -2, -3)
    assert (A.DV_MAX_DEPTH, A.DV_MAX_SPEC, A.DV_MAX_CODE, A.DV_MAX_CLI) == (const("MAX_DEPTH"), const("MAX_SPEC"), const("MAX_CODE"), const("MAX_CLI")) == \
        (32, 1024, 65536, 512)
    assert (A.DV_KIND_DERIVE, A.DV_KIND_CROSS) == (const("KIND_DERIVE"), const("KIND_CROSS"))
    for method in ("derive_masks", "derive_timing"):
        assert callable(getattr(api.PrecisionRecall, method))
    assert callable(api.derive_compile) and callable(api.derive_cross) and callable(RP.write_derived_strata)
    # the header says what the bits mean: a border variant is in !x, and which names cannot be named
    assert "x and !x partition the hap-variants" in hdr and "cannot be named" in hdr and "not on intervals" in hdr


def test_wellformed_arguments_are_planned():
    args = CLI.parse(["q.vcf", "t.vcf", "ref.fa"] + OTHERS + [D, "easy=!*", X, "ins_*,del_*:hp_*", D, "dm=!(hp_ge12|snp_ti)", X, "easy:hom"])
    assert args.stratify_derive == ["easy=!*", "dm=!(hp_ge12|snp_ti)"] and args.stratify_cross == ["ins_*,del_*:hp_*", "easy:hom"]
    plan = CLI.plan_strata(args)
    dv = plan.derived
    # every stratum of the families first, then the derived entries in command-line order, then the crossed pairs option by option
    assert plan.names[:25] == DC.NAMES and plan.names[25:27] == ["easy", "dm"] and plan.names[27] == "ins_1to5&hp_4to6" and plan.names[-1] == "easy&hom"
    assert len(plan.names) == 25 + 2 + 24 + 1 and dv.names == plan.names[25:]
    assert dv.kinds == [A.DV_KIND_DERIVE] * 2 + [A.DV_KIND_CROSS] * 25 and dv.expressions[:3] == ["!*", "!(hp_ge12|snp_ti)", "ins_1to5&hp_4to6"]
    assert dv.code_off[0] == 0 and len(dv.code_off) == 28 and dv.code_off[-1] == len(dv.code) and dv.code[-3:] == [25, DC.K["hom"], A.DV_AND]
    tot = CLI.Totals(args, plan)
    assert tot.dv_members.shape == (2, 27) and tot.tally[-1] is tot.dv_members and tot.vs_members.shape == (2, 14)
    # without the options nothing of it is there
    args = CLI.parse(["q.vcf", "t.vcf", "ref.fa"] + OTHERS)
    plan = CLI.plan_strata(args)
    tot = CLI.Totals(args, plan)
    assert args.stratify_derive == [] and plan.derived.names == [] and tot.dv_members is None and all(a is not None for a in tot.tally)
    assert not CLI.stratifying(CLI.parse(["q.vcf", "t.vcf", "ref.fa", D, "x=hom"]))         # (--cut-classes keeps its own requirement)


def refused_alike(tmp_path, options, want):
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa")]
    with pytest.raises(SystemExit) as e:
        CLI.main(missing + options)
    assert str(e.value) == want
    r = subprocess.run([GPU_CLI] + missing + options, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr == want + "\n" and r.stdout == ""


@pytest.mark.parametrize("value,what", DC.MALFORMED, ids=[m[0][:40] for m in DC.MALFORMED])
def test_both_drivers_refuse_a_malformed_derive_alike(tmp_path, value, what):
    refused_alike(tmp_path, OTHERS + [D, value], f"ERROR: {D}: entry '{value}': {what}")


@pytest.mark.parametrize("value,what", DC.MALFORMED_CROSS, ids=[m[0] for m in DC.MALFORMED_CROSS])
def test_both_drivers_refuse_a_malformed_cross_alike(tmp_path, value, what):
    refused_alike(tmp_path, OTHERS + [X, value], f"ERROR: {X}: entry '{value}': {what}")


def test_references_between_entries(tmp_path):
    # an entry names the entries in front of it, not itself, not a later one; a derived entry cannot name a crossed stratum
    refused_alike(tmp_path, OTHERS + [D, "p=q", D, "q=hom"], f"ERROR: {D}: entry 'p=q': unknown stratum 'q'" + DC.U)
    refused_alike(tmp_path, OTHERS + [D, "q=hom", D, "p=q|p"], f"ERROR: {D}: entry 'p=q|p': 'p' is the entry itself")
    plan = CLI.plan_strata(CLI.parse(["q.vcf", "t.vcf", "ref.fa"] + OTHERS + [X, "hom:het", D, "p=*"]))
    assert plan.names[25:] == ["p", "hom&het"] and plan.derived.code[:plan.derived.code_off[1]] == DC.union_code(range(25))
    # a name twice: against a default name, against an earlier derived entry, a pair twice
    refused_alike(tmp_path, OTHERS + [D, "q=hom", D, "q=het"], f"ERROR: {D}: entry 'q=het': name 'q' is already a stratum")
    refused_alike(tmp_path, ["--stratify-variants", D, "near_10=hom"], f"ERROR: {D}: entry 'near_10=hom': name 'near_10' is already a stratum")
    refused_alike(tmp_path, OTHERS + [X, "hom:het", X, "ho*:he*"], f"ERROR: {X}: entry 'ho*:he*': name 'hom&het' is already a stratum")
    # a context name is unknown where only the variant strata are on
    refused_alike(tmp_path, ["--stratify-variants", D, "x=hp_ge12"], f"ERROR: {D}: entry 'x=hp_ge12': unknown stratum 'hp_ge12'" + DC.U)


def test_a_name_of_the_list_is_refused(tmp_path):
    (tmp_path / "a.bed").write_text("chr1\t10\t20\n")
    lst = tmp_path / "list.tsv"
    lst.write_text("whole\ta.bed\nodd\ta.bed\n")
    refused_alike(tmp_path, ["--stratify", str(lst), D, "odd=!whole"], f"ERROR: {D}: entry 'odd=!whole': name 'odd' is already a stratum")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa")]
    with pytest.raises(Exception) as e:             # (with another name the plan is fine: the first input does not exist)
        CLI.main(missing + ["--stratify", str(lst), D, "even=!odd", X, "even:whole"])
    assert "no_query" in str(e.value)


@pytest.mark.parametrize("options,option", [([D, "x=hom"], D), ([X, "hom:het"], X), ([D, "x=hom", X, "hom:het"], D),
                                            ([D, "x=hom", "--bootstrap", "4"], D)])
def test_the_options_need_another_stratify_option(tmp_path, options, option):
    refused_alike(tmp_path, options, f"ERROR: {option} needs another --stratify* option")


def test_more_than_512_strata_are_refused(tmp_path):
    # 50 derived entries and 14 x 11 = 154 pairs three times (by name where a glob would take in a crossed stratum's name): 512
    copies = [a for k in range(50) for a in (D, f"c{k}=hom")]
    context = ",".join(DC.CONTEXT)
    fill = [X, "snp_*,ins_*,del_*,hom,het,iso_50,near_10:hp_*,tr_*,gc_*", X, ",".join(f"c{k}" for k in range(14)) + ":" + context,
            X, ",".join(f"c{k}" for k in range(14, 28)) + ":" + context]
    assert 50 + 3 * 154 == 512
    args = CLI.parse(["q.vcf", "t.vcf", "ref.fa"] + OTHERS + copies + fill)
    assert len(CLI.plan_strata(args).derived.names) == 512                        # the limit itself is planned
    refused_alike(tmp_path, OTHERS + copies + fill + [X, "hom:het"], f"ERROR: {X}: more than 512 derived and crossed strata")
    refused_alike(tmp_path, OTHERS + copies + [D, "one_more=het"] + fill, f"ERROR: {X}: more than 512 derived and crossed strata")
