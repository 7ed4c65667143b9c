"""Variant strata on the GPU (include/vcfdist_varstrata.h, pr_varstrata.hip): the membership words against the brute-force model
of tests/varstrata_model.py (hand cases, a random batch over two contigs, slots of 0, 1, 257 and 513 variants), appending behind
BED, context and uploaded words, the stratified counters and a bootstrap pass against strata_model / bootstrap_model, the state
machine of the calls, and both command lines with --stratify-variants on one and on two ranks."""
import copy
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
import strata_model as M
import varstrata_cases as VC
import varstrata_model as VM
from vcfdist_amd import _abi as A
from vcfdist_amd import api, io as IO, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def masks(pr, v, specs, **kw):
    pr.varstrata_masks(v, specs, **kw)
    return pr.download_strata_masks()


def check_words(got, want, v):
    for h in range(4):
        assert got[h].shape == want[h].shape and got[h].shape[1] == v.n_vars(h), (h, got[h].shape, want[h].shape)
        assert np.array_equal(got[h], want[h]), (h, np.nonzero(got[h] != want[h]))


# ---- 1. words

def test_hand_cases_equal_the_model():
    v = VC.hand_case()
    names, specs = VC.hand_specs()
    bits = VM.members(v, specs)
    assert all(any(b[k].any() for b in bits) for k in range(len(specs)))          # every entry has a member
    pr = api.PrecisionRecall()
    check_words(masks(pr, v, specs), [VM.words_of(b) for b in bits], v)
    assert pr.varstrata_timing() > 0
    # every entry alone, and the set in reverse order: no bit depends on its neighbours in the spec
    check_words(masks(pr, v, specs[::-1]), [VM.words_of(b[::-1]) for b in bits], v)
    for k in (0, 10, 11, 12, 13, 17):
        check_words(masks(pr, v, specs[k:k + 1]), [VM.words_of(b[k:k + 1]) for b in bits], v)


@pytest.fixture(scope="module")
def random_batch():
    names, specs = api.varstrata_default()
    v = VC.random_variants()
    return v, specs, VM.members(v, specs)


def test_random_batch_equals_the_model(random_batch):
    v, specs, bits = random_batch
    q, t = VM.member_counts(bits)
    assert (q > 0).all() and (t > 0).all()                                           # no default stratum is vacuous, in either callset
    assert [v.n_vars(h) for h in range(4)] == [513, 257, 640, 300]
    pr = api.PrecisionRecall()
    got = masks(pr, v, specs)
    check_words(got, [VM.words_of(b) for b in bits], v)
    check_words(masks(pr, v, specs), got, v)                                         # a second call gives identical words
    # one query variant without a partner slot, 513 truth variants on one hap: an empty slot, the tail of a workgroup
    e = VC.edge_variants()
    assert [e.n_vars(h) for h in range(4)] == [1, 0, 513, 0]
    check_words(masks(pr, e, specs), [VM.words_of(b) for b in VM.members(e, specs)], e)
    # 64 entries fill a word
    names64, specs64 = VC.hand_specs()
    specs64 = (specs64 * 3)[:64]
    check_words(masks(pr, e, specs64), [VM.words_of(b) for b in VM.members(e, specs64)], e)


# ---- 2. appending

@pytest.fixture(scope="module")
def beds(tmp_path_factory):
    """70 random BED strata over the random batch's two contigs"""
    rng = np.random.RandomState(5)
    strata = [(f"s{k}", CC.random_rows(rng, "c0", 100000) + CC.random_rows(rng, "c1", 100000)) for k in range(70)]
    names, beds = IO.read_strata(M.write_strata(tmp_path_factory.mktemp("varstrata_beds"), strata))
    return beds


@pytest.mark.parametrize("n_bed", [0, 58, 70])
def test_append_behind_bed_strata(random_batch, beds, n_bed):
    v, specs, bits = random_batch
    pr = api.PrecisionRecall()
    old = None
    if n_bed:
        pr.strata_masks(v, M.strata_of(beds[:n_bed], ["c0", "c1"]))
        old = pr.download_strata_masks()
        assert any(o.any() for o in old)
    got = masks(pr, v, specs, append=n_bed > 0)
    check_words(got, [VM.words_of(bits[h], n_bed, old[h] if n_bed else None) for h in range(4)], v)
    if n_bed:       # the old bits are unchanged, bit for bit
        low = np.uint64((1 << (n_bed & 63)) - 1)
        for h in range(4):
            assert np.array_equal(got[h][:n_bed >> 6], old[h][:n_bed >> 6]) and np.array_equal(got[h][n_bed >> 6] & low, old[h][n_bed >> 6] & low)
    if n_bed == 58:     # the strata 58..71 straddle the first word boundary
        assert all(g.shape[0] == 2 for g in got) and any(g[1].any() for g in got) and any((g[0] >> np.uint64(58)).any() for g in got)
    if n_bed == 70:     # a second append follows the first
        again = masks(pr, v, specs[:3], append=True)
        check_words(again, [VM.words_of(bits[h][:3], 84, got[h]) for h in range(4)], v)


def test_append_behind_context_and_uploaded_words(random_batch, beds):
    v, specs, bits = random_batch
    ctx_names, ctx = api.context_default()
    pr = api.PrecisionRecall()
    pr.context_masks(v, ctx, M.strata_of(beds[:50], ["c0", "c1"]))
    old = pr.download_strata_masks()
    assert any((o[0] >> np.uint64(50)).any() for o in old)                            # a context stratum has a member
    got = masks(pr, v, specs, append=True)                                            # 61 + 14 strata
    check_words(got, [VM.words_of(bits[h], 61, old[h]) for h in range(4)], v)
    assert any(g[1].any() for g in got)
    # behind words made elsewhere: 63 strata of random bits
    rng = np.random.RandomState(9)
    up = [rng.randint(0, 1 << 62, size=(1, v.n_vars(h))).astype(np.uint64) for h in range(4)]
    pr.upload_strata_masks(63, up)
    got = masks(pr, v, specs, append=True)
    check_words(got, [VM.words_of(bits[h], 63, up[h]) for h in range(4)], v)


# ---- 3. counters

@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    """an evaluated synthetic batch with three BED strata and the default variant strata appended behind them"""
    syn = VC.synth()
    v = syn.variants()
    batch = api.batch_from_variants(v)
    names, specs = api.varstrata_default()
    bits = VM.members(v, specs)
    rng = np.random.RandomState(2)
    length = int(v.ctg_off[1])
    strata = [(f"r{k}", CC.random_rows(rng, "c0", length) or [("c0", 0, length)]) for k in range(3)]
    _, beds = IO.read_strata(M.write_strata(tmp_path_factory.mktemp("varstrata_counts"), strata))
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold=6) for s in range(4)]
    pb, _, _ = S.phase(res.sc_phase, np.ones(batch.n_sc, np.int32))
    plain = S.pr_counts(pr, cls, pb)
    pr.strata_masks(v, M.strata_of(beds, ["c0"]))
    bed_counts = S.pr_counts_strata(pr, cls, pb)
    pr.varstrata_masks(v, specs, append=True)
    return dict(v=v, batch=batch, specs=specs, bits=bits, pr=pr, res=res, cls=cls, pb=pb, plain=plain, bed_counts=bed_counts)


def test_counters_equal_the_oracle(counted):
    c = counted
    pr, batch, res, cls, pb, bits = c["pr"], c["batch"], c["res"], c["cls"], c["pb"], c["bits"]
    got = S.pr_counts_strata(pr, cls, pb)
    assert got.shape[0] == 17 and np.array_equal(got[:3], c["bed_counts"])            # the BED strata count what they counted
    for k in range(14):
        want = M.expected_counts(batch.var_off, res, cls, pb, [bits[s][k] for s in range(4)])
        assert np.array_equal(got[3 + k], want), k
    assert all(got[3 + k].any() for k in (0, 1, 2, 6, 10, 11, 12, 13))
    # hom and het partition the variants
    assert np.array_equal(got[3 + 10] + got[3 + 11], c["plain"]) and c["plain"].any()
    # a bootstrap pass cut by a variant stratum
    keys = A.boot_keys(0, np.arange(batch.n_sc))
    for k in (10, 13):
        boot = pr.pr_counts_boot(None, pb, keys, 33, 7, stratum=3 + k)
        member = [bits[s][k] for s in range(4)]
        assert boot.any() and np.array_equal(boot, BM.expected_counts(batch.var_off, res, cls, pb, keys, 7, 33, member=member)), k


def test_transitions_and_transversions_partition_snps():
    v = VC.synth(snp_only=True).variants()
    batch = api.batch_from_variants(v)
    names, specs = api.varstrata_default()
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s]) for s in range(4)]
    pb, _, _ = S.phase(res.sc_phase, np.ones(batch.n_sc, np.int32))
    plain = S.pr_counts(pr, cls, pb)
    pr.varstrata_masks(v, specs)
    got = S.pr_counts_strata(pr, cls, pb)
    assert got.shape[0] == 14 and got[0].any() and got[1].any() and not got[2:10].any()
    assert np.array_equal(got[0] + got[1], plain) and np.array_equal(got[10] + got[11], plain)


# ---- 4. state and arguments

def test_state_and_arguments(random_batch):
    v, specs, bits = random_batch
    pr = api.PrecisionRecall()

    def refused(code, *a, **kw):
        with pytest.raises(api.VprError) as e:
            pr.varstrata_masks(*a, **kw)
        assert f"({code})" in str(e.value) and "vpr_varstrata_masks" in str(e.value), str(e.value)
        return str(e.value)
    # append without resident words
    assert "append without resident membership words" in refused(-4, v, specs, append=True)
    # an unsorted var_pos, a decreasing sc_ctg
    bad = copy.deepcopy(v)
    i = int(np.nonzero(np.diff(bad.var_pos[2][:200]) > 0)[0][5])
    bad.var_pos[2][[i, i + 1]] = bad.var_pos[2][[i + 1, i]]
    msg = refused(-1, bad, specs)
    assert "hap slot 2" in msg and "var_pos is unsorted" in msg and f"variant {i + 1} " in msg, msg
    bad = copy.deepcopy(v)
    bad.sc_ctg[200] = 0
    assert "sc_ctg decreases at supercluster 200" in refused(-1, bad, specs)
    bad = copy.deepcopy(v)
    bad.sc_ctg[299] = 2
    assert "supercluster 299 names contig 2" in refused(-1, bad, specs)
    # spec entries outside their limits: the message names the entry
    Z, N, K = A.vs_size, A.vs_near, A.VprVariantStratum
    for b in (Z(A.TYPE_SUB, 1), Z(A.TYPE_INS, 0), Z(A.TYPE_DEL, 5, 4), N(-1, 0), N(5, -1), N(5, 3, 2), N(5, 0, -2), K(6, 0, 0, 0, 0, 0, 0),
              K(-1, 0, 0, 0, 0, 0, 0)):
        assert "entry 1" in refused(-1, v, [specs[0], b]), b
    assert "n_spec 0" in refused(-1, v, []) and "n_spec 65" in refused(-1, v, [specs[0]] * 65)
    with pytest.raises(api.VprError):
        pr.download_strata_masks()                                                    # no failed call left words behind
    # append with other variant counts
    pr.upload_strata_masks(3, [np.zeros((1, n), np.uint64) for n in (513, 257, 640, 299)])
    msg = refused(-4, v, specs, append=True)
    assert "hap slot 3" in msg and "299" in msg and "300" in msg, msg
    assert pr.download_strata_masks()[3].shape == (1, 299)                            # (the resident words are still there)
    # the limits themselves are accepted; after the refusals the handle still makes the right words
    got = masks(pr, v, [Z(A.TYPE_INS, 1, 1), N(0, 0, 0), N(2 ** 31 - 1, 0)] + [specs[10]] * 61)
    assert all(g.shape[0] == 1 for g in got)
    check_words(masks(pr, v, specs), [VM.words_of(b) for b in bits], v)
    # the words go with the next upload, as those of vpr_strata_masks
    pr.upload(api.batch_from_variants(VC.synth().variants()))
    with pytest.raises(api.VprError):
        pr.download_strata_masks()
    assert "append without resident membership words" in refused(-4, v, specs, append=True)


# ---- 5. the command lines

STRAT_FILES = ("stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv")
STRAT_BOOT = "stratified-bootstrap-precision-recall-summary.tsv"
VS_FILE = "variant-strata.tsv"


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
def demo():
    """the demo callsets through the CPU oracle chain (tests/demo_pipeline.py), the model's bits of the default set on its variant
    tables, and the text of the stratified tables and of variant-strata.tsv they give"""
    import demo_pipeline as D
    import report_oracle as RO
    from vcfdist_amd import cluster as K
    rows, det = D.run(product=False)
    sc, slots, fasta = det["sc"], det["slots"], det["fasta"]
    haps = [K.HapSeq(s["pos"], s["type"], s["ref"], s["alt"]) for s in slots]
    v = A.Variants(np.array([0, len(fasta)], np.int64), fasta, np.zeros(sc.n, np.int32), sc.beg, sc.end, [sc.var_off(i) for i in range(4)],
                   [h.pos for h in haps], [h.type for h in haps], [np.asarray(s["qual"], np.float32) for s in slots], [h.ref_off for h in haps],
                   [h.ref_len for h in haps], [h.alt_off for h in haps], [h.alt_len for h in haps], [h.pool for h in haps])
    names, specs = api.varstrata_default()
    bits = VM.members(v, specs)
    cls = [S.var_class(h.type, h.ref_len, h.alt_len, D.G["sv_threshold"]) for h in haps]
    all_rows, sum_rows = [], []
    for k, name in enumerate(names):
        counts = M.expected_counts(det["batch"].var_off, det["res"], cls, det["pb"], [bits[s][k] for s in range(4)], D.G["min_qual"], D.G["max_qual"])
        a, s = RO.precision_recall(counts, D.G["min_qual"], D.G["max_qual"])
        all_rows += [name + "\t" + l + "\n" for l in a.split("\n")[1:-1]]
        sum_rows += [name + "\t" + l + "\n" for l in s.split("\n")[1:-1]]
        head = ("STRATUM\t" + a.split("\n")[0] + "\n", "STRATUM\t" + s.split("\n")[0] + "\n")
    q, t = VM.member_counts(bits)
    # superclusters whose variants of one callset lie within 50 bases of the next supercluster's: NEAR and HOM look across the edge
    close = 0
    for cs in (0, 2):
        first = [min(int(v.var_pos[s][v.var_off[s][k]]) if v.var_off[s][k] < v.var_off[s][k + 1] else 1 << 40 for s in (cs, cs + 1)) for k in range(sc.n)]
        last = [max(int(v.var_pos[s][v.var_off[s][k + 1] - 1]) if v.var_off[s][k] < v.var_off[s][k + 1] else -1 << 40 for s in (cs, cs + 1)) for k in range(sc.n)]
        close += sum(1 for k in range(sc.n - 1) if first[k + 1] - last[k] <= 50)
    return dict(names=names, specs=specs, bits=bits, files={STRAT_FILES[0]: head[1] + "".join(sum_rows), STRAT_FILES[1]: head[0] + "".join(all_rows),
                                                                VS_FILE: VM.tsv_text(names, specs, q, t)}, members=(q, t), close=close)


def test_command_lines_on_demo_files(demo, tmp_path):
    import demo_pipeline as D
    names = demo["names"]
    assert (demo["members"][0][[0, 1, 2, 6, 10, 11, 12, 13]] > 0).all() and (demo["members"][1][[0, 1, 2, 6, 10, 11, 12, 13]] > 0).all()
    fa = _write_fasta(tmp_path / "surrogate.fa", D.surrogate_fasta(5_100_000), ("chr1",))
    iv = [l.split("\t")[:3] for l in open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")).read().split("\n") if l]
    iv = [("chr1", int(a), int(b)) for _, a, b in iv]
    beds = M.write_strata(tmp_path, [("whole", [("chr1", 0, 5_000_000)]), ("even", iv[0::2]), ("odd", iv[1::2])], "beds.tsv")
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    boot = ["--bootstrap", "16"]
    every = ["--stratify", beds, "--stratify-context", "--stratify-variants"]
    runs = {}
    for name, cmd, extra in (("c", cli, []), ("c-v", cli, ["--stratify-variants"] + boot), ("py-v", py, ["--stratify-variants"] + boot),
                             ("c-bxv", cli, every), ("py-bxv", py, every[::-1][:2] + every[:2]), ("c-n", cli, ["--stratify-variants", "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    # the stratified tables and variant-strata.tsv: byte-identical from both drivers, and what the model and the oracle give
    for f in STRAT_FILES + (VS_FILE,):
        assert rd(runs["c-v"][0] + f) == rd(runs["py-v"][0] + f), f
        assert rd(runs["c-v"][0] + f).decode() == demo["files"][f], f
    assert rd(runs["c-v"][0] + STRAT_BOOT) == rd(runs["py-v"][0] + STRAT_BOOT) and len(rd(runs["c-v"][0] + STRAT_BOOT)) > 500
    for name in ("c-bxv", "py-bxv"):
        assert rd(runs[name][0] + VS_FILE).decode() == demo["files"][VS_FILE], name
    # with the list and the context strata as well: list, context, variants; no part changes another's rows
    ctx_names = api.context_default()[0]
    for f in STRAT_FILES:
        assert rd(runs["c-bxv"][0] + f) == rd(runs["py-bxv"][0] + f), f
        lines = open(runs["c-bxv"][0] + f).read().split("\n")
        order = [l.split("\t", 1)[0] for l in lines[1:-1]]
        assert [n for i, n in enumerate(order) if i == 0 or order[i - 1] != n] == ["whole", "even", "odd"] + ctx_names + names, f
        assert [l for l in lines[1:-1] if l.split("\t", 1)[0] in names] == demo["files"][f].split("\n")[1:-1], f
        whole = "".join(l.split("\t", 1)[1] + "\n" for l in lines[:-1] if l.startswith(("STRATUM\t", "whole\t")))
        assert whole == open(runs["c-bxv"][0] + f.replace("stratified-", "")).read(), f
    # the run without the option is unchanged: every file of the plain run, and stdout
    plain = sorted(os.listdir(runs["c"][0]))
    assert VS_FILE not in plain and sorted(set(os.listdir(runs["c-v"][0])) - set(STRAT_FILES) - {VS_FILE, STRAT_BOOT, "bootstrap-precision-recall-summary.tsv",
                                                                                              "bootstrap-replicates.tsv"}) == plain
    for name in ("c-v", "c-bxv"):
        for f in plain:
            assert _without_command(runs["c"][0] + f) == _without_command(runs[name][0] + f), (name, f)
    assert runs["c"][1] == runs["c-v"][1] == runs["py-v"][1] == runs["c-bxv"][1] == runs["py-bxv"][1] == runs["c-n"][1]
    assert "stratified" not in runs["c"][2] and "variant strata" not in runs["c"][2]
    # stderr: the stratified line with the larger count, and one more line with the variant strata and their device time
    for name, n in (("c-v", 14), ("py-v", 14), ("c-bxv", 28), ("py-bxv", 28), ("c-n", 14)):
        m = re.findall(r"stratified: (\d+) strata, (\d+) of (\d+) hap-variants in none of them", runs[name][2])
        assert len(m) == 1 and int(m[0][0]) == n and int(m[0][1]) == 0 < int(m[0][2]), runs[name][2][-500:]      # (hom or het: never none)
        m = re.findall(r"variant strata: 14 strata, ([0-9.]+) ms on the device", runs[name][2])
        assert len(m) == 1 and float(m[0]) > 0, runs[name][2][-500:]
    assert os.listdir(runs["c-n"][0]) == []                                   # -n: no file appears
    # a variant-stratum name that is also a name of the list ends the run before anything is evaluated
    bad = tmp_path / "bad.tsv"
    bad.write_text("whole\twhole.bed\nins_ge50\teven.bed\n")
    for cmd in (cli, py):
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad), "--stratify-variants"], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and "duplicate stratum name 'ins_ge50'" in r.stderr and "PRECISION-RECALL" not in r.stdout


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the demo callsets twice, as chr1 and chr2 (the inputs of tests/test_gpu_strata.py's two-rank test), a BED strata list over
    both contigs, and the one-rank run with --stratify, --stratify-variants and --bootstrap"""
    import gzip
    import demo_pipeline as D
    tmp = tmp_path_factory.mktemp("varstrata_two")
    fa = _write_fasta(tmp / "two.fa", D.surrogate_fasta(5_100_000), ("chr1", "chr2"))

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
    base = [str(qv), str(tv), fa, "-b", str(bed), "--stratify", lst, "--stratify-variants", "--bootstrap", "8"]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    return tmp, base, env


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(two_contigs, demo, how):
    tmp, base, env = two_contigs
    assert demo["close"] > 100            # superclusters closer than 50 bases: dealt over the ranks, NEAR and HOM cross a shard's edge
    out = tmp / how
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # (the child runs under its own time limit: a rank that hangs in a collective is ended, not waited for)
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vcfdist_amd"] + base + ["-p", str(out) + "/", "--shard", how],
                   check=True, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=660)
    for name in STRAT_FILES + (STRAT_BOOT, VS_FILE, "precision-recall.tsv", "precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    # both contigs hold the demo callsets: every stratum has twice the demo's members
    q, t = demo["members"]
    assert (out / VS_FILE).read_text() == VM.tsv_text(demo["names"], demo["specs"], 2 * q, 2 * t)
    text = (out / STRAT_FILES[0]).read_text()
    assert "whole\tALL\tNONE" in text and "near_10\tSNP\tBEST" in text and "hom\tINDEL\tBEST" in text
