"""The branches of the C++ command line (vcfdist_amd/csrc/main.cpp) that no other test reaches, with every option at once on the
three small contigs of tests/cli_paths_cases.py: a contig only the truth VCF has records on, a contig without a record (zero
superclusters: the context intervals alone), -n, and realignment with distance clustering.  Both drivers write the same bytes."""
import os
import re
import socket
import subprocess
import sys

import pytest
import torch  # noqa: F401 -- before the library is loaded: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import cli_paths_cases as PC
import context_model as CM
import longrepeats_model as LM
import repeats_model as RM
from label_common import ROOT, _without_command
from vcfdist_amd import api

pytestmark = pytest.mark.gpu

REPLICATES = 4


def every_option(w):
    return ["-d", "--stratify", w["list"], "--stratify-repeats", "--stratify-long-repeats", "--stratify-context", "--stratify-variants",
            "--bootstrap", str(REPLICATES), "--classify-errors", "--classify-matches", "--cut-classes"]


def test_every_option_on_three_contigs(tmp_path):
    w = PC.write(tmp_path)
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    every = every_option(w)
    runs = {}
    for name, cmd, extra in (("c", cli, every), ("py", py, every), ("c-n", cli, every + ["-n"]), ("c-r", cli, ["-rq", "-rt", "-c", "gap", "50"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(["timeout", "-k", "10", "120"] + cmd + w["inputs"] + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT,
                           timeout=150)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        runs[name] = (pre, r.stdout, r.stderr)
    # every file both drivers write, byte for byte
    files = sorted(os.listdir(runs["c"][0]))
    assert files == sorted(os.listdir(runs["py"][0])) and len(files) > 30, (files, sorted(os.listdir(runs["py"][0])))
    for f in files:
        assert _without_command(runs["c"][0] + f) == _without_command(runs["py"][0] + f), f
    assert runs["c"][1] == runs["py"][1] == runs["c-n"][1] and "PRECISION-RECALL SUMMARY" in runs["c"][1] and "ALL" in runs["c"][1]
    assert os.listdir(runs["c-n"][0]) == []                                   # -n: no file appears
    for f in ("orig-query.vcf", "orig-truth.vcf", "query.vcf", "truth.vcf", "summary.vcf"):
        assert os.path.getsize(runs["c-r"][0] + f) > 100, f
    assert all(f"realigned {which} VCF: " in runs["c-r"][2] for which in ("query", "truth"))

    # stderr of the C++ driver: the contig only the truth VCF has, the contig without a record, and one closing line per option
    err = runs["c"][2]
    assert "Contig 'chrB' found in truth VCF but not query VCF" in err
    assert "chrC: 0 hap-variants, 0 clusters, 0 superclusters" in err
    n_a = PC.hap_variants(PC.CHR_A, True) + PC.hap_variants(PC.CHR_A, False)
    assert f"chrA: {n_a} hap-variants" in err and f"chrB: {PC.hap_variants(PC.CHR_B, False)} hap-variants" in err
    ctgs = w["contigs"]
    rep, lrep, ctx, vs = api.repeats_default(), api.longrepeats_default(), api.context_default(), api.varstrata_default()
    n_strata = len(PC.STRATA) + len(rep[0]) + len(lrep[0]) + len(ctx[0]) + len(vs[0])
    one = lambda pattern: (re.findall(pattern, err) + [None, None])[:2]
    m, more = one(r"stratified: (\d+) strata, (\d+) of (\d+) hap-variants in none of them")
    assert more is None and (int(m[0]), int(m[2])) == (n_strata, n_a + PC.hap_variants(PC.CHR_B, False)), err[-3000:]
    for word, model, (names, specs) in (("repeat", RM, rep), ("long repeat", LM, lrep)):
        rows = model.all_intervals(ctgs, specs)[0]
        m, more = one(rf"\] {word} strata: (\d+) intervals of (\d+) strata, ")
        assert more is None and (int(m[0]), int(m[1])) == (sum(len(r[c][0]) for r in rows for c in range(3)), len(names)), (word, err[-3000:])
    ctx_rows = CM.all_intervals(ctgs, ctx[1])
    m, more = one(r"context strata: (\d+) intervals of (\d+) strata, ")
    assert more is None and (int(m[0]), int(m[1])) == (sum(len(r[c][0]) for r in ctx_rows for c in range(3)), len(ctx[0])), err[-3000:]
    m, more = one(r"variant strata: (\d+) strata, ")
    assert more is None and int(m) == len(vs[0]), err[-3000:]
    m, more = one(r"error classes: window 50, (\d+) query FP and (\d+) truth FN classified, ")
    assert more is None and int(m[0]) >= 1 and int(m[1]) >= 1 + PC.hap_variants(PC.CHR_B, False), err[-3000:]   # (2201; 1301 and all of chrB)
    m, more = one(r"match kinds: query TP (\d+) exact, .* truth TP (\d+) exact, ")
    assert more is None and int(m[0]) > 0 and int(m[1]) > 0, err[-3000:]
    for noun in ("error classes", "match kinds"):
        m, more = one(rf"{noun} cut: (\d+) strata, (\d+) replicates, ")
        assert more is None and (int(m[0]), int(m[1])) == (n_strata, REPLICATES), (noun, err[-3000:])
    m, more = one(r"bootstrap: (\d+) replicates, seed (\d+), ")
    assert more is None and (int(m[0]), int(m[1])) == (REPLICATES, 1), err[-3000:]

    # context-strata.bed lists rows for all three contigs: the model's text (the contig without a record included)
    assert open(runs["c"][0] + "context-strata.bed").read() == CM.context_bed_text(ctx[0], PC.NAMES, ctx_rows)
    assert {l.split("\t")[0] for l in open(runs["c"][0] + "context-strata.bed").read().split("\n") if l} == set(PC.NAMES)
    # variant-strata.tsv counts the truth members on the contig the query lacks: every hap-variant is either hom or het
    rows = [l.split("\t") for l in open(runs["c"][0] + "variant-strata.tsv").read().split("\n")[1:] if l]
    hom_het = [r for r in rows if r[1] in ("HOM", "HET")]
    assert len(hom_het) == 2
    assert sum(int(r[8]) for r in hom_het) == PC.hap_variants(PC.CHR_A, True)
    assert sum(int(r[9]) for r in hom_het) == PC.hap_variants(PC.CHR_A, False) + PC.hap_variants(PC.CHR_B, False)


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """the three contigs and the Python driver's one-rank run with every option but -d (distance is refused on several ranks)
    -> (directory, the arguments without the prefix, the environment, the one-rank run's stdout)"""
    tmp = tmp_path_factory.mktemp("cli_paths_ranks")
    w = PC.write(tmp)
    base = w["inputs"] + every_option(w)[1:]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    (tmp / "one").mkdir()
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    return tmp, base, env, r.stdout


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_two_ranks_every_option(one_rank, how):
    """every section of the vector the ranks sum at once (strata, variant members, replicates, both label passes and their cuts),
    with a contig of which a rank's share is empty: the files and the summary are the one-rank run's"""
    tmp, base, env, summary = one_rank
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base +
                       ["-p", str(out) + "/", "--shard", how], capture_output=True, text=True, env=env, cwd=ROOT, timeout=330)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(tmp / "one"))
    assert files == sorted(os.listdir(out)) and len(files) > 25, (files, sorted(os.listdir(out)))
    for f in files:
        assert _without_command(str(tmp / "one" / f)) == _without_command(str(out / f)), f
    # stdout ends with the summary, and in front of it stands nothing but what gloo announces there when the group comes up, long
    # before: "[Gloo] Rank 0 is connected to 1 peer ranks. Expected number of connected peer ranks is : 1" once per rank, each written
    # in pieces that the two ranks' lines interleave -- so the head is to consist of that line's words, numbers and blanks alone
    assert r.stdout.endswith(summary) and "PRECISION-RECALL SUMMARY" in summary
    head = r.stdout[:len(r.stdout) - len(summary)]
    words = r"\[Gloo\]|Rank|is|connected|to|peer|ranks\.|Expected|number|of|ranks|:|[0-9]+|\s+"
    assert re.sub(words, "", head) == "", r.stdout[:400]
