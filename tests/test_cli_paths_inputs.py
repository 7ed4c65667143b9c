"""The inputs of tests/test_gpu_cli_paths.py (tests/cli_paths_cases.py) hold what that test is about, checked without a GPU: every
default repeat, long repeat and context stratum has an interval on the three contigs, and the contigs play their three roles."""
import context_model as CM
import longrepeats_model as LM
import repeats_model as RM
from vcfdist_amd import api

import cli_paths_cases as PC


def test_every_default_stratum_has_an_interval():
    ctgs = PC.contigs()
    assert len(ctgs) == 3 and all(len(c) == PC.LENGTH for c in ctgs)
    for what, model, (names, specs) in (("repeat", RM, api.repeats_default()), ("long repeat", LM, api.longrepeats_default())):
        rows = model.all_intervals(ctgs, specs)[0]
        n = {name: [len(r[c][0]) for c in range(3)] for name, r in zip(names, rows)}
        assert all(min(v) > 0 for v in n.values()), (what, n)          # (on every contig: the copies span all three)
    names, specs = api.context_default()
    n = {name: sum(len(r[c][0]) for c in range(3)) for name, r in zip(names, CM.all_intervals(ctgs, specs))}
    assert len(n) == 11 and all(v > 0 for v in n.values()), n


def test_the_three_contig_roles(tmp_path):
    w = PC.write(tmp_path)
    body = lambda p: [l.split("\t") for l in open(p).read().split("\n") if l and not l.startswith("#")]
    head = lambda p: [l for l in open(p).read().split("\n") if l.startswith("##contig")]
    q, t = body(w["inputs"][0]), body(w["inputs"][1])
    for p in w["inputs"][:2]:
        assert [h.split("ID=")[1].split(",")[0] for h in head(p)] == PC.NAMES               # both headers name all three
    # chrA: a dozen records in both callsets -- SNPs, an insertion, a deletion, a het/hom mismatch, two PS values
    qa, ta = [r for r in q if r[0] == "chrA"], [r for r in t if r[0] == "chrA"]
    assert len(qa) == 12 and len(ta) == 12 and {r[0] for r in q} == {"chrA"}
    for rows in (qa, ta):
        assert sum(len(r[3]) == 1 and len(r[4]) == 1 for r in rows) == 10
        assert sum(len(r[3]) == 1 and len(r[4]) == 3 for r in rows) == 1 and sum(len(r[3]) == 3 and len(r[4]) == 1 for r in rows) == 1
        assert len({r[9].split(":")[1] for r in rows}) == 2 and all("|" in r[9] for r in rows)
    gt = lambda rows: {r[1]: r[9].split(":")[0] for r in rows}
    assert gt(ta)["1901"] == "1|1" and gt(qa)["1901"] == "0|1"
    assert set(gt(ta)) - set(gt(qa)) == {"1301"} and set(gt(qa)) - set(gt(ta)) == {"2201"}
    # every REF is the FASTA's
    for r in q + t:
        c = w["contigs"][PC.NAMES.index(r[0])]
        assert c[int(r[1]) - 1:int(r[1]) - 1 + len(r[3])].decode() == r[3] and r[4] != r[3], r
    # chrB: the truth VCF only; chrC: the BED and the headers, no record
    assert [r[0] for r in t if r[0] != "chrA"] == ["chrB"] * 3 and PC.hap_variants(PC.CHR_B, False) == 4 and PC.hap_variants(PC.CHR_B, True) == 0
    assert [l.split("\t")[0] for l in open(w["inputs"][4]).read().split("\n") if l] == PC.NAMES
    inside = {c: (a, b) for c, a, b in PC.BED}
    assert all(inside[r[0]][0] <= int(r[1]) - 1 and int(r[1]) - 1 + len(r[3]) <= inside[r[0]][1] for r in q + t)
    assert len([l for l in open(w["list"]).read().split("\n") if l and not l.startswith("#")]) == 2
