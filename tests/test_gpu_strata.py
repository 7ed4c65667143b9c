"""Region-stratified precision/recall counters on the GPU (include/vcfdist_strata.h, pr_strata.hip, pr_cut.hip): the membership words
against the host's vio_bed_contains, the stratified counters against the counting oracle, the state machine of the calls,
the native collective, and both command lines with --stratify (one rank and two)."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import strata_model as M
from vcfdist_amd import _abi as A
from vcfdist_amd import api, io as IO, summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB, INS, DEL = A.TYPE_SUB, A.TYPE_INS, A.TYPE_DEL


def _beds(tmp, strata):
    """strata: [(name, rows)] -> [IO.Bed] read back through the strata list reader"""
    names, beds = IO.read_strata(M.write_strata(tmp, strata))
    assert names == [n for n, _ in strata]
    return beds


# ---- 1. membership edge cases

def test_membership_edge_cases(tmp_path):
    contigs = ["A" * 80, "C" * 80]
    sites = [(p, SUB, "A", "G") for p in (9, 10, 19, 20, 29, 30, 39, 40, 49, 50)]
    sites += [(a, DEL, "A" * (b - a), "") for a, b in ((5, 10), (18, 22), (25, 45), (30, 40), (45, 55), (12, 15))]
    sites += [(p, INS, "", "T") for p in (10, 15, 19, 20, 49, 50)]
    # (nothing is executed here: one variant per supercluster, dealt over the four hap slots)
    scs = [dict(ctg=0, beg=max(p - 1, 0), end=p + len(r) + 1,
                vars=[[(p, t, r, a, 30.0)] if h == i % 4 else [] for h in range(4)]) for i, (p, t, r, a) in enumerate(sites)]
    v = A.Variants.from_sites(contigs, scs)
    names = ["c0", "c1"]
    beds = _beds(tmp_path, [("regions", [("c0", 10, 20), ("c0", 20, 30), ("c0", 40, 50)]), ("whole", [("c0", 0, 80), ("c1", 0, 80)]),
                            ("other_contig_of_the_batch", [("c1", 10, 70)]), ("foreign_contig", [("chrOther", 0, 1000)])])
    loc = M.locations(beds, names, v)
    seen = set(np.concatenate([l.ravel() for l in loc]).tolist())
    assert seen == {M.INSIDE, M.BORDER, M.OUTSIDE, M.OFFCTG}, seen            # (not a vacuous pass)
    flat = {(int(v.var_pos[h][0]), int(v.var_type[h][0]), int(v.var_ref_len[h][0])): int(loc[h][0][0])
            for h in range(4)}     # spot checks of the specification itself, on the first variant of each slot
    assert flat[(9, SUB, 1)] == M.OUTSIDE and flat[(10, SUB, 1)] == M.INSIDE
    pr = api.PrecisionRecall()
    pr.strata_masks(v, M.strata_of(beds, names))
    got = pr.download_strata_masks()
    for h in range(4):
        want = M.words_of(loc[h])
        assert got[h].shape == want.shape == (1, v.n_vars(h))
        assert np.array_equal(got[h], want), (h, got[h], want)
        assert (got[h][0] >> np.uint64(1) & np.uint64(1)).all() and not (got[h][0] >> np.uint64(2)).any()


# ---- 2. random masks

def _three_contigs():
    """a synthetic workload spread over three contigs (the same sequence three times; supercluster k lies on contig k % 3)"""
    syn = api.Synth(n_sc=600, len_a=10, len_b=300, len_max=300, seed=7, var_per_base=0.02)
    v = syn.variants()
    n = int(v.ctg_off[1])
    v.ctg_off = np.array([0, n, 2 * n, 3 * n], np.int64)
    v.ctg_seq = np.ascontiguousarray(np.tile(v.ctg_seq, 3))
    v.sc_ctg = (np.arange(v.n_sc) % 3).astype(np.int32)
    return v, n


def _random_rows(rng, ctg, length):
    """0 - 200 sorted non-overlapping regions of one contig, about one gap in twenty closed (abutting regions)"""
    n = int(rng.choice([0, 0, 1, 2, 17, 200, rng.randint(0, 201)]))
    if n == 0:
        return []
    cuts = np.sort(rng.choice(np.arange(1, length), size=2 * n, replace=False))
    st, sp = cuts[0::2].copy(), cuts[1::2].copy()
    close = np.nonzero(rng.rand(n - 1) < 0.05)[0]
    sp[close] = st[close + 1]
    return [(ctg, int(a), int(b)) for a, b in zip(st, sp)]


@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    v, length = _three_contigs()
    names = ["c0", "c1", "c2"]
    rng = np.random.RandomState(5)
    strata = []
    for k in range(70):
        rows = [r for c in names for r in _random_rows(rng, c, length)]
        if k == 3:
            rows = [("elsewhere", 0, 10)]
        strata.append((f"s{k}", rows))
    beds = _beds(tmp_path_factory.mktemp("random_strata"), strata)
    loc = M.locations(beds, names, v)
    return v, M.strata_of(beds, names), [M.words_of(l) for l in loc], loc


@pytest.mark.parametrize("level_b", [False, True])
def test_random_masks_equal_the_model(random_case, level_b):
    v, strata, want, loc = random_case
    assert sum(v.n_vars(h) for h in range(4)) > 3000 and {1, 2, 3} <= set(np.concatenate(v.var_type).tolist())
    assert all((l == k).any() for l in loc for k in (M.INSIDE, M.BORDER, M.OUTSIDE, M.OFFCTG))
    assert strata.n_strata == 70 and (np.diff(strata.iv_off) == 0).any() and (strata.iv_start[1:] == strata.iv_stop[:-1]).any()
    pr = api.PrecisionRecall()
    if level_b:
        pr.upload_variants(v.as_struct(), v)
        pr.execute()
    else:
        pr.run(api.batch_from_variants(v))
    pr.strata_masks(v, strata)
    got = pr.download_strata_masks()
    for h in range(4):
        assert got[h].shape == (2, v.n_vars(h))
        assert np.array_equal(got[h], want[h]), (h, np.nonzero(got[h] != want[h]))
    assert any(w[1].any() for w in want)         # strata beyond the first word have members


# ---- 3. counts

@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    """the batch of tests/test_summary.py::test_device_counts_and_summary_against_oracle, executed once, and 70 strata:
    0 the whole contig, 1 empty, 2-4 a three-way tiling of the contig, 5-69 random"""
    syn = api.Synth(n_sc=4000, len_mode=1, len_a=25.0, len_b=1.0, len_min=4, len_max=2000, seed=31, p_keep=0.8, p_drop=0.1)
    v = syn.variants()
    batch = syn.batch()
    pr = api.PrecisionRecall()
    res = pr.run(batch)
    cls = [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold=6) for s in range(4)]
    pb, _, _ = S.phase(res.sc_phase, np.ones(batch.n_sc, np.int32))
    length = int(v.ctg_off[1])
    # the tiles' first cut lies inside a counted truth deletion, so that the model reports a BORDER variant
    dels = np.nonzero((v.var_type[2] == DEL) & (v.var_ref_len[2] >= 2) & (res.errtype[2][0] < 3) & (res.errtype[2][1] < 3) &
                      (v.var_pos[2] > length // 4))[0]
    cut1 = int(v.var_pos[2][dels[0]]) + 1
    cut2 = (cut1 + length) // 2
    rng = np.random.RandomState(9)
    strata = [("whole", [("c0", 0, length)]), ("empty", [("elsewhere", 0, length)]),
              ("tile0", [("c0", 0, cut1)]), ("tile1", [("c0", cut1, cut2)]), ("tile2", [("c0", cut2, length)])]
    strata += [(f"r{k}", _random_rows(rng, "c0", length) or [("c0", 7, length // 3)]) for k in range(65)]
    beds = _beds(tmp_path_factory.mktemp("count_strata"), strata)
    loc = M.locations(beds, ["c0"], v)
    return dict(v=v, batch=batch, pr=pr, res=res, cls=cls, pb=pb, beds=beds, loc=loc)


@pytest.mark.parametrize("quals", [(0, 60), (10, 40)])
@pytest.mark.parametrize("n_strata", [1, 33, 70])
def test_stratified_counts_equal_the_oracle(counted, n_strata, quals):
    c = counted
    pr, v, batch, res, cls, pb, loc = c["pr"], c["v"], c["batch"], c["res"], c["cls"], c["pb"], c["loc"]
    min_qual, max_qual = quals
    pr.strata_masks(v, M.strata_of(c["beds"][:n_strata], ["c0"]))
    got = S.pr_counts_strata(pr, cls, pb, min_qual, max_qual)
    assert got.shape == (n_strata, 2, 4, 3, max_qual - min_qual + 1)
    total = S.pr_counts(pr, cls, pb, min_qual, max_qual)
    want = [M.expected_counts(batch.var_off, res, cls, pb, [loc[s][k] == M.INSIDE for s in range(4)], min_qual, max_qual)
            for k in range(n_strata)]
    for k in range(n_strata):
        assert np.array_equal(got[k], want[k]), k
    # (a) the whole contig: exactly vpr_pr_counts and the oracle
    assert all((loc[s][0] == M.INSIDE).all() for s in range(4))
    assert np.array_equal(got[0], total) and total[:, 3].sum() > 0
    assert np.array_equal(total, M.O.oracle_pr_counts(M.O.lib(), batch.var_off, res, cls, pb, min_qual, max_qual))
    if n_strata == 1:
        return
    # (b) an empty stratum
    assert not got[1].any()
    # (d) the tiling: never more than the total, and less exactly where the model says a variant sits on a border
    tiles = got[2:5].sum(axis=0)
    assert (tiles <= total).all()
    border = any((loc[s][2:5] == M.BORDER).any() for s in range(4))
    assert border and not np.array_equal(tiles, total)
    assert np.array_equal(tiles, sum(want[2:5]))
    # (c) random strata: they differ from each other and from the total
    assert len({g.tobytes() for g in got[5:]}) > (n_strata - 5) // 3 and any(g.any() for g in got[5:])


# ---- 4. state and arguments

def test_state_and_arguments(counted, tmp_path):
    c = counted
    v, cls, pb = c["v"], c["cls"], c["pb"]
    pr = api.PrecisionRecall()
    pr.run(c["batch"])
    strata = M.strata_of(c["beds"][:7], ["c0"])

    def refused(code, f, *a, **kw):
        with pytest.raises(api.VprError) as e:
            f(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)
    refused(-4, S.pr_counts_strata, pr, cls, pb)                # counts before any masks: VPR_ERR_STATE
    refused(-1, pr.strata_masks, v, A.Strata([], 1))            # n_strata = 0: VPR_ERR_ARG
    refused(-1, pr.strata_masks, v, A.Strata([[([50, 10], [60, 20])]], 1))       # unsorted
    refused(-1, pr.strata_masks, v, A.Strata([[([10, 19], [20, 30])]], 1))       # overlapping
    refused(-1, pr.strata_masks, v, A.Strata([[([10], [10])]], 1))               # stop <= start
    refused(-1, pr.strata_masks, v, A.Strata([[([10], [20]), ([10], [20])]], 2)) # another contig numbering than the variants'
    pr.strata_masks(v, A.Strata([[([10, 20], [20, 30])]], 1))                    # abutting regions are allowed
    # masks of another batch: VPR_ERR_STATE at the counts call
    other = api.Synth(n_sc=50, len_a=10, len_b=300, len_max=300, seed=3, var_per_base=0.02).variants()
    pr.strata_masks(other, A.Strata([[([10], [2000])]], 1))
    refused(-4, S.pr_counts_strata, pr, cls, pb)
    # the real ones; two calls give identical output; a further execute of the same batch keeps the words
    pr.strata_masks(v, strata)
    one = S.pr_counts_strata(pr, cls, pb)
    assert one.any() and np.array_equal(one, S.pr_counts_strata(pr, None, pb))
    pr.execute()
    assert np.array_equal(one, S.pr_counts_strata(pr, cls, pb))
    # downloaded words uploaded again: the same counts
    words = pr.download_strata_masks()
    pr.strata_masks(other, A.Strata([[([10], [2000])]], 1))
    pr.upload_strata_masks(7, words)
    assert np.array_equal(one, S.pr_counts_strata(pr, cls, pb))
    assert all(np.array_equal(a, b) for a, b in zip(words, pr.download_strata_masks()))
    # the next upload releases the words: VPR_ERR_STATE again
    pr.run(c["batch"])
    refused(-4, S.pr_counts_strata, pr, cls, pb)
    refused(-4, pr.download_strata_masks)


# ---- 5. native collective

def test_native_collective_on_a_one_rank_communicator(counted):
    from vcfdist_amd import rccl
    if not rccl.available():
        pytest.skip("no RCCL library in this process")
    torch.cuda.set_device(0)
    c = counted
    pr = c["pr"]
    pr.strata_masks(c["v"], M.strata_of(c["beds"][:40], ["c0"]))
    comm = rccl.Comm(1, 0, rccl.unique_id())
    try:
        want = S.pr_counts_strata(pr, c["cls"], c["pb"])
        got = rccl.allreduce_counts_strata(pr, comm, c["cls"], c["pb"])
        assert want.sum() > 0 and np.array_equal(got, want)
    finally:
        comm.destroy()


# ---- 6, 7. the command lines

STRAT_FILES = ("stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv")


def _demo_strata(tmp, contigs=("chr1",)):
    """the whole of chr1:0-5 000 000 and two BEDs cut from the demo BED's own intervals (the even and the odd ones)"""
    import demo_pipeline as D
    iv = [l.split("\t")[:3] for l in open(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")).read().split("\n") if l]
    iv = [(int(a), int(b)) for _, a, b in iv]
    rows = lambda part: [(c, a, b) for c in contigs for a, b in part]
    return M.write_strata(tmp, [("whole", rows([(0, 5_000_000)])), ("even", rows(iv[0::2])), ("odd", rows(iv[1::2]))])


def _without_command(path):
    """a file's bytes without the lines that record the command line, the output prefix or the date (parameters.txt: command,
    out_prefix; summary.vcf: ##CL, ##fileDate): two runs into two directories differ there whatever their options"""
    return b"\n".join(l for l in open(path, "rb").read().split(b"\n") if not l.startswith((b"##fileDate", b"##CL=", b"command = ", b"out_prefix = ")))


def _surrogate(tmp_path, contigs=("chr1",)):
    import demo_pipeline as D
    fa = tmp_path / "surrogate.fa"
    s = bytes(D.surrogate_fasta(5_100_000)).decode()
    with open(fa, "w") as fh:
        for c in contigs:
            fh.write(f">{c}\n")
            for i in range(0, len(s), 100000):
                fh.write(s[i:i + 100000] + "\n")
    return str(fa)


def test_command_lines_on_demo_files(tmp_path):
    import demo_pipeline as D
    fa = _surrogate(tmp_path)
    lst = _demo_strata(tmp_path)
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    runs = {}
    for name, cmd, extra in (("c", [cli], []), ("c-s", [cli], ["--stratify", lst]), ("py-s", [sys.executable, "-m", "vcfdist_amd"], ["--stratify", lst]),
                             ("c-n", [cli], ["--stratify", lst, "-n"])):
        pre = str(tmp_path / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    rd = lambda p: open(p, "rb").read()
    for f in STRAT_FILES:
        assert rd(runs["c-s"][0] + f) == rd(runs["py-s"][0] + f), f          # the C++ files equal the Python driver's
        assert not os.path.exists(runs["c"][0] + f)
    # the whole-contig stratum reproduces the unstratified tables of the same run, text for text
    for name in ("c-s", "py-s"):
        for f in STRAT_FILES:
            lines = open(runs[name][0] + f).read().split("\n")
            whole = "".join(l.split("\t", 1)[1] + "\n" for l in lines[:-1] if l.startswith(("STRATUM\t", "whole\t")))
            assert whole == open(runs[name][0] + f.replace("stratified-", "")).read(), (name, f)
            assert {l.split("\t", 1)[0] for l in lines[1:-1]} == {"whole", "even", "odd"}
    summary = [l.split("\t") for l in open(runs["c-s"][0] + STRAT_FILES[0]).read().split("\n")[1:-1]]
    none_all = {r[0]: [int(x) for x in r[4:8]] for r in summary if r[1] == "ALL" and r[2] == "NONE"}
    assert all(sum(v) > 0 for v in none_all.values())
    assert all(none_all["even"][i] + none_all["odd"][i] <= none_all["whole"][i] for i in range(4))
    # every other output file, and stdout, equal the run without --stratify
    plain = sorted(os.listdir(runs["c"][0]))
    assert sorted(set(os.listdir(runs["c-s"][0])) - set(STRAT_FILES)) == plain
    for f in plain:
        assert _without_command(runs["c"][0] + f) == _without_command(runs["c-s"][0] + f), f
    assert runs["c"][1] == runs["c-s"][1] == runs["py-s"][1]
    # one line on stderr: the number of strata and of hap-variants in none
    for name in ("c-s", "py-s", "c-n"):
        m = re.findall(r"stratified: 3 strata, (\d+) of (\d+) hap-variants in none of them", runs[name][2])
        assert len(m) == 1 and 0 <= int(m[0][0]) < int(m[0][1]), runs[name][2][-500:]
    assert os.listdir(runs["c-n"][0]) == [] and runs["c-n"][1] == runs["c"][1]           # -n: no stratified file appears
    # a faulty list ends the run before anything is evaluated
    bad = tmp_path / "bad.tsv"
    bad.write_text("whole\twhole.bed\nwhole\teven.bed\n")
    for cmd in ([cli], [sys.executable, "-m", "vcfdist_amd"]):
        r = subprocess.run(cmd + inputs + ["-n", "--stratify", str(bad)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and "duplicate stratum name 'whole'" in r.stderr and "PRECISION-RECALL" not in r.stdout


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the inputs of tests/test_demo_known_answer.py::test_command_line_two_ranks (the demo callsets twice, as chr1 and chr2), a
    strata list over both contigs, and the one-rank run"""
    import gzip
    import demo_pipeline as D
    tmp = tmp_path_factory.mktemp("two_contigs")
    fa = _surrogate(tmp, ("chr1", "chr2"))

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
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    base = [str(qv), str(tv), fa, "-b", str(bed), "--stratify", _demo_strata(tmp, ("chr1", "chr2"))]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    return tmp, base, env


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(two_contigs, how):
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
    for name in STRAT_FILES + ("precision-recall.tsv", "precision-recall-summary.tsv"):
        one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
        assert one == two and len(one) > 60, name
    text = (out / STRAT_FILES[0]).read_text()
    assert "whole\tALL\tNONE" in text and "odd\tSNP\tBEST" in text
