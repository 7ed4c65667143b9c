"""Sequence-context strata on the GPU (include/vcfdist_context.h, pr_context.hip): the intervals against the numpy model of
tests/context_model.py (hand contigs, kernel seams), the membership words and the stratified counters over BED plus context
strata against strata_model, the state machine of the calls, and both command lines with --stratify-context."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import bootstrap_model as BM
import context_cases as CC
import context_model as CM
import strata_model as M
from vcfdist_amd import _abi as A
from vcfdist_amd import api, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def variants_on(contigs):
    """an A.Variants over the given contig sequences without any variant (the interval kernels read ctg_off / ctg_seq only)"""
    return A.Variants.from_sites([c if isinstance(c, str) else bytes(c).decode() for c in contigs], [])


def check_rows(got, want):
    assert len(got) == len(want) and all(len(g) == len(w) for g, w in zip(got, want))
    bad = CM.same(got, want)
    assert not bad, [(k, c, [x.tolist() for x in got[k][c]], [x.tolist() for x in want[k][c]]) for k, c in bad[:3]]
    for row in (r for per in got for r in per):
        assert row[0].dtype == np.int32 and (row[1] > row[0]).all() and (row[0][1:] > row[1][:-1]).all()      # sorted, merged, non-empty


# ---- 1. hand contigs

def test_hand_contigs_equal_the_model():
    contigs, specs = CC.hand_case()
    want = CM.all_intervals(contigs, specs)
    sizes = [len(r[0]) for per in want for r in per]
    assert 0 in sizes and max(sizes) > 0                       # an empty (stratum, contig) row and one that is not
    pr = api.PrecisionRecall()
    pr.context_masks(variants_on(contigs), specs)
    check_rows(pr.download_context_intervals(), want)
    # the same contigs in reverse order, and each one alone: no state of a neighbour leaks
    pr.context_masks(variants_on(contigs[::-1]), specs)
    check_rows(pr.download_context_intervals(), [per[::-1] for per in want])
    for c in (0, 3, 4, 8):
        pr.context_masks(variants_on(contigs[c:c + 1]), specs)
        check_rows(pr.download_context_intervals(), [per[c:c + 1] for per in want])


# ---- 2. seams

def test_seams_equal_the_model(monkeypatch):
    pr = api.PrecisionRecall()
    bpw, bpl = pr.context_info()
    assert (bpw, bpl) == api.context_info() and bpw % bpl == 0
    contigs, specs = CC.seam_case(bpw, bpl)
    want = CM.all_intervals(contigs, specs)
    seams = CC.seam_positions(bpw, bpl)
    assert CC.intervals_cover(want[0], seams, "start") == set(seams) == CC.intervals_cover(want[1], seams, "stop")
    v = variants_on(contigs)
    pr.context_masks(v, specs)
    one = pr.download_context_intervals()
    check_rows(one, want)
    ms = pr.context_timing()
    assert ms[0] > 0
    pr.context_masks(v, specs)                                  # a second call gives identical arrays
    two = pr.download_context_intervals()
    assert not CM.same(two, one)
    # the genome in pieces of one contig each: the same rows
    monkeypatch.setenv("VPR_CONTEXT_PIECE_BASES", "100000")
    pr.context_masks(v, specs)
    check_rows(pr.download_context_intervals(), want)


def test_wide_gc_windows_equal_the_model():
    """windows around the width up to which the kernel keeps its counts in LDS, and far beyond it"""
    bpw, bpl = api.context_info()
    contigs, _ = CC.seam_case(bpw, bpl)
    contigs = [contigs[2][:40011], contigs[0][:5000], contigs[1][:25000]]
    specs = [A.ctx_gc(49, 50, 8192, 0), A.ctx_gc(50, 51, 8193, 2), A.ctx_gc(0, 101, 20000, 3), A.ctx_gc(49, 50, 4097, 0), A.ctx_gc(50, 101, 9001, 0)]
    want = CM.all_intervals(contigs, specs)
    assert all(any(len(r[0]) for r in per) for per in want) and any(len(r[0]) > 3 for per in want for r in per)
    pr = api.PrecisionRecall()
    pr.context_masks(variants_on(contigs), specs)
    check_rows(pr.download_context_intervals(), want)


# ---- 3. words, 4. counters

@pytest.fixture(scope="module")
def words(tmp_path_factory):
    return CC.words_case(tmp_path_factory.mktemp("context_words"))


@pytest.mark.parametrize("n_bed", [70, 58, 0])
@pytest.mark.parametrize("level_b", [False, True])
def test_words_equal_the_model(words, level_b, n_bed):
    w = words
    v, loc, beds, specs = w["v"], w["loc"], w["beds"], w["specs"]
    assert len(beds) == 81 and len(specs) == 11
    ctx = [l[70:] for l in loc]
    assert all(any((c[k] == M.INSIDE).any() for c in ctx) for k in range(11))       # every context stratum has a member
    assert any((c == M.BORDER).any() for c in ctx)
    pr = api.PrecisionRecall()
    if level_b:
        pr.upload_variants(v.as_struct(), v)
        pr.execute()
    else:
        pr.run(api.batch_from_variants(v))
    pr.context_masks(v, specs, M.strata_of(beds[:n_bed], ["c0"]) if n_bed else None)
    got = pr.download_strata_masks()
    n_strata = n_bed + 11
    for h in range(4):
        want = M.words_of(np.concatenate([loc[h][:n_bed], loc[h][70:]]))
        assert got[h].shape == want.shape == ((n_strata + 63) // 64, v.n_vars(h))
        assert np.array_equal(got[h], want), (h, np.nonzero(got[h] != want))
    check_rows(pr.download_context_intervals(), w["rows"])
    if n_bed == 58:          # the context strata 58..68 straddle the first word boundary
        assert any(g[1].any() for g in got) and any((g[0] >> np.uint64(58)).any() for g in got)
    if n_bed == 70:          # the BED strata are exactly the words of vpr_strata_masks
        pr.strata_masks(v, M.strata_of(beds[:70], ["c0"]))
        alone = pr.download_strata_masks()
        low = np.uint64((1 << 6) - 1)
        assert all(np.array_equal(a[0], g[0]) and np.array_equal(a[1], g[1] & low) for a, g in zip(alone, got))


def test_counters_equal_the_oracle(words):
    w = words
    v, loc, beds, specs = w["v"], w["loc"], w["beds"], w["specs"]
    batch = api.batch_from_variants(v)
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold=6) for s in range(4)]
    pb, _, _ = S.phase(res.sc_phase, np.ones(batch.n_sc, np.int32))
    pr.context_masks(v, specs, M.strata_of(beds[:70], ["c0"]))
    got = S.pr_counts_strata(pr, cls, pb)
    assert got.shape[0] == 81
    for k in range(81):
        want = M.expected_counts(batch.var_off, res, cls, pb, [loc[s][k] == M.INSIDE for s in range(4)])
        assert np.array_equal(got[k], want), k
    assert all(got[k].any() for k in range(70, 81))
    # one context stratum through the bootstrap's stratum cut
    keys = A.boot_keys(0, np.arange(batch.n_sc))
    k = 72
    boot = pr.pr_counts_boot(None, pb, keys, 33, 7, stratum=k)
    member = [loc[s][k] == M.INSIDE for s in range(4)]
    assert boot.any() and np.array_equal(boot, BM.expected_counts(batch.var_off, res, cls, pb, keys, 7, 33, member=member))


# ---- 5. state and arguments

def test_state_and_arguments(words):
    w = words
    v, specs = w["v"], w["specs"]
    pr = api.PrecisionRecall()

    def refused(code, f, *a, **kw):
        with pytest.raises(api.VprError) as e:
            f(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)
        return str(e.value)
    refused(-4, pr.download_context_intervals)                   # before any call: VPR_ERR_STATE
    L = api.lib()
    assert L.vpr_context_download_intervals(pr._h, None, None) == -4
    P, G = A.ctx_period, A.ctx_gc
    bad = [P(0, 4), P(7, 9), P(2, 2), P(1, 4, 3), P(1, 4, 0, -1), G(-1, 10, 5), G(30, 30, 5), G(50, 102, 5), G(0, 50, 0), G(0, 50, 5, -2),
           A.VprContextStratum(2, 1, 4, 0, 0, 0, 0, 0)]
    for b in bad:
        msg = refused(-1, pr.context_masks, v, [specs[0], b])
        assert "entry 1" in msg, msg
    refused(-1, pr.context_masks, v, [])
    refused(-1, pr.context_masks, v, [specs[0]] * 65)
    refused(-1, pr.context_masks, v, specs, A.Strata([[([50, 10], [60, 20])]], 1))        # a faulty BED table is refused as by strata_masks
    refused(-4, pr.download_context_intervals)                   # a failed call leaves no intervals
    pr.context_masks(v, [specs[0]] * 64)                         # the limit itself
    rows = pr.download_context_intervals()
    assert len(rows) == 64 and not CM.same(rows, [w["rows"][0]] * 64)
    # after a failed call the handle still evaluates a batch correctly, and the intervals outlive the upload
    refused(-1, pr.context_masks, v, [P(0, 4)])
    batch = api.batch_from_variants(v)
    res = pr.run(batch)
    other = api.PrecisionRecall()
    assert not res.diff(other.run(batch))
    refused(-4, pr.download_strata_masks)                        # the words went with the upload
    pr.context_masks(v, specs)
    pr.upload(batch)
    assert not CM.same(pr.download_context_intervals(), w["rows"])
    refused(-4, pr.download_strata_masks)


# ---- 6. the command lines

STRAT_FILES = ("stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv")
STRAT_BOOT = "stratified-bootstrap-precision-recall-summary.tsv"
CONTEXT_BED = "context-strata.bed"


def _without_command(path):
    """a file's bytes without the lines that record the command line, the output prefix or the date"""
    return b"\n".join(l for l in open(path, "rb").read().split(b"\n") if not l.startswith((b"##fileDate", b"##CL=", b"command = ", b"out_prefix = ")))


def _write_fasta(path, seq, contigs):
    s = bytes(seq).decode()
    with open(path, "w") as fh:
        for c in contigs:
            fh.write(f">{c}\n")
            for i in range(0, len(s), 100000):
                fh.write(s[i:i + 100000] + "\n")
    return str(path)


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """the surrogate FASTA with planted tracts, the model's intervals of the default set on it, and those as BEDs plus a list"""
    tmp = tmp_path_factory.mktemp("context_demo")
    seq, sites = CC.demo_fasta()
    names, specs = api.context_default()
    rows = CM.all_intervals([seq], specs)
    assert all(len(r[0][0]) > 0 for r in rows)                 # every default stratum has an interval
    return dict(tmp=tmp, seq=seq, sites=sites, names=names, specs=specs, rows=rows)


def test_command_lines_on_demo_files(demo, tmp_path):
    import demo_pipeline as D
    names, rows = demo["names"], demo["rows"]
    fa = _write_fasta(tmp_path / "surrogate.fa", demo["seq"], ("chr1",))
    lst, _ = CM.write_model_strata(tmp_path, names, ["chr1"], rows)
    iv = [l.split("\t")[:3] for l in open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")).read().split("\n") if l]
    iv = [("chr1", int(a), int(b)) for _, a, b in iv]
    beds = M.write_strata(tmp_path, [("whole", [("chr1", 0, 5_000_000)]), ("even", iv[0::2]), ("odd", iv[1::2])], "beds.tsv")
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    boot = ["--bootstrap", "16"]
    runs = {}
    for name, cmd, extra in (("c", cli, []), ("c-x", cli, ["--stratify-context"] + boot), ("py-x", py, ["--stratify-context"] + boot),
                             ("c-l", cli, ["--stratify", lst] + boot), ("c-bx", cli, ["--stratify", beds, "--stratify-context"]),
                             ("py-bx", py, ["--stratify-context", "--stratify", beds]), ("c-n", cli, ["--stratify-context", "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    # context-strata.bed equals the model; the C++ and the Python files are byte-identical
    want_bed = CM.context_bed_text(names, ["chr1"], rows).encode()
    for name in ("c-x", "py-x", "c-bx", "py-bx"):
        assert rd(runs[name][0] + CONTEXT_BED) == want_bed, name
    for f in STRAT_FILES + (STRAT_BOOT,):
        assert rd(runs["c-x"][0] + f) == rd(runs["py-x"][0] + f), f
        # the end-to-end check: the same tables as --stratify LIST over the model's BEDs under the same names
        assert rd(runs["c-x"][0] + f) == rd(runs["c-l"][0] + f) and len(rd(runs["c-x"][0] + f)) > 500, f
    assert not os.path.exists(runs["c-l"][0] + CONTEXT_BED) and not os.path.exists(runs["c"][0] + CONTEXT_BED)
    # every default stratum has a member
    summary = [l.split("\t") for l in open(runs["c-x"][0] + STRAT_FILES[0]).read().split("\n")[1:-1]]
    none_all = {r[0]: [int(x) for x in r[4:8]] for r in summary if r[1] == "ALL" and r[2] == "NONE"}
    assert list(none_all) == names and all(sum(v) > 0 for v in none_all.values()), none_all
    # with --stratify as well the BED strata come first, and neither part changes the other's rows
    for f in STRAT_FILES:
        assert rd(runs["c-bx"][0] + f) == rd(runs["py-bx"][0] + f), f
        lines = open(runs["c-bx"][0] + f).read().split("\n")
        order = [l.split("\t", 1)[0] for l in lines[1:-1]]
        assert [n for i, n in enumerate(order) if i == 0 or order[i - 1] != n] == ["whole", "even", "odd"] + names, f
        ctx_rows = [l for l in lines[1:-1] if l.split("\t", 1)[0] in names]
        assert ctx_rows == open(runs["c-x"][0] + f).read().split("\n")[1:-1], f
        whole = "".join(l.split("\t", 1)[1] + "\n" for l in lines[:-1] if l.startswith(("STRATUM\t", "whole\t")))
        assert whole == open(runs["c-bx"][0] + f.replace("stratified-", "")).read(), f
    # the run without the option is unchanged: every file of the plain run, and stdout
    plain = sorted(os.listdir(runs["c"][0]))
    assert sorted(set(os.listdir(runs["c-bx"][0])) - set(STRAT_FILES) - {CONTEXT_BED}) == plain
    for name in ("c-x", "c-bx"):
        for f in plain:
            assert _without_command(runs["c"][0] + f) == _without_command(runs[name][0] + f), (name, f)
    assert runs["c"][1] == runs["c-x"][1] == runs["py-x"][1] == runs["c-bx"][1] == runs["c-n"][1]
    assert "stratified" not in runs["c"][2] and "context" not in runs["c"][2]
    # stderr: the stratified line with the larger count, and a second line with the intervals and their device time
    n_iv = sum(len(r[0][0]) for r in rows)
    for name, n in (("c-x", 11), ("py-x", 11), ("c-bx", 14), ("py-bx", 14), ("c-n", 11)):
        m = re.findall(r"stratified: (\d+) strata, (\d+) of (\d+) hap-variants in none of them", runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == n and 0 <= int(m[0][1]) < int(m[0][2]), runs[name][2][-500:]
        m = re.findall(r"context strata: (\d+) intervals of 11 strata, ([0-9.]+) ms on the device", runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == n_iv and float(m[0][1]) > 0, runs[name][2][-500:]
    assert os.listdir(runs["c-n"][0]) == []                                   # -n: no file appears
    # a context name that collides with a name of the list ends the run before anything is evaluated
    bad = tmp_path / "bad.tsv"
    bad.write_text("whole\twhole.bed\nhp_ge12\teven.bed\n")
    for cmd in (cli, py):
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad), "--stratify-context"], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and "duplicate stratum name 'hp_ge12'" in r.stderr and "PRECISION-RECALL" not in r.stdout
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-500:]                             # (the list alone is fine)


@pytest.fixture(scope="module")
def two_contigs(demo):
    """the demo callsets twice, as chr1 and chr2 (the inputs of tests/test_gpu_strata.py's two-rank test) on the planted FASTA,
    a BED strata list over both contigs, and the one-rank run with --stratify, --stratify-context and --bootstrap"""
    import gzip
    import demo_pipeline as D
    tmp = demo["tmp"]
    fa = _write_fasta(tmp / "two.fa", demo["seq"], ("chr1", "chr2"))

    def twice(lines):
        head = [l for l in lines if l.startswith("#")]
        body = [l for l in lines if l and not l.startswith("#")]
        head = [l for l in head if not l.startswith("##contig")] or head
        ctg = ["##contig=<ID=chr1,length=5100000>", "##contig=<ID=chr2,length=5100000>"]
        return "\n".join(head[:1] + ctg + head[1:] + body + ["chr2" + l[4:] for l in body if l.startswith("chr1\t")]) + "\n"
    qv, tv, bed = tmp / "q.vcf", tmp / "t.vcf", tmp / "r.bed"
    qv.write_text(twice(open(os.path.join(D.DEMO, "query.vcf")).read().split("\n")))
    tv.write_text(twice(gzip.open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), "rt").read().split("\n")))
    b = [l for l in open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")).read().split("\n") if l]
    bed.write_text("\n".join(b + ["chr2" + l[4:] for l in b]) + "\n")
    lst = M.write_strata(tmp, [("whole", [(c, 0, 5_000_000) for c in ("chr1", "chr2")])], "two.tsv")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    base = [str(qv), str(tv), fa, "-b", str(bed), "--stratify", lst, "--stratify-context", "--bootstrap", "8"]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    return tmp, base, env


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(two_contigs, demo, how):
    tmp, base, env = two_contigs
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base + ["-p", str(out) + "/", "--shard", how],
                   check=True, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=660)
    for name in STRAT_FILES + (STRAT_BOOT, CONTEXT_BED, "precision-recall.tsv", "precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    assert (out / CONTEXT_BED).read_text() == CM.context_bed_text(demo["names"], ["chr1", "chr2"], [[r[0], r[0]] for r in demo["rows"]])
    text = (out / STRAT_FILES[0]).read_text()
    assert "whole\tALL\tNONE" in text and "hp_4to6\tINDEL\tBEST" in text and "gc_30to55\tSNP\tBEST" in text
