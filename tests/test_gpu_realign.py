"""The realignment (-rq / -rt / -ro) on the GPU: vrl_realign's columns and cluster status against the CPU model
(tests/realign_model.py), every column bit for bit, on seeded synthetic callsets of the wgs_synth and joint_synth shapes, with
other penalties, many rounds, the keep-original path and two calls; then both command lines on the demo files."""
import datetime
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import realign_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu

WGS = dict(n_sc=25000, seed=3, len_mode=1, len_a=20.0, len_b=1.2, len_min=4, len_max=10000)
JOINT = dict(n_sc=1500, seed=11, len_mode=1, len_a=20.0, len_b=1.2, len_min=4, len_max=10002, p_sv=0.1, sv_min=50, sv_max=3000)


def callsets(params, slot=0, gap=50):
    """query hap 1 of a synthetic batch as a callset: per contig the hap (with seeded PS / GQ / GT columns), its gap clusters and
    the contig"""
    from vcfdist_amd import api, cluster as K
    v = api.Synth(**params).variants()
    rng = np.random.RandomState(params["seed"])
    out = []
    for c in range(len(v.ctg_off) - 1):
        scs = np.nonzero(v.sc_ctg == c)[0]
        if len(scs) == 0:
            continue
        a, b = int(v.var_off[slot][scs[0]]), int(v.var_off[slot][scs[-1] + 1])
        n = b - a
        if n == 0:
            continue
        hap = dict(pos=v.var_pos[slot][a:b].copy(), type=v.var_type[slot][a:b].copy(), ref_len=v.var_ref_len[slot][a:b].copy(),
                   alt_len=v.var_alt_len[slot][a:b].copy(), ref_off=v.var_ref_off[slot][a:b].copy(), alt_off=v.var_alt_off[slot][a:b].copy(),
                   pool=v.allele_pool[slot].copy(),
                   var_qual=(v.var_qual[slot][a:b] + rng.rand(n).astype(np.float32) * 0.9).astype(np.float32),
                   phase_set=np.where(rng.rand(n) < 0.3, 0, rng.randint(1, 5, n) * 1000).astype(np.int32),
                   gt_qual=rng.randint(0, 99, n).astype(np.float32), orig_gt=rng.randint(3, 6, n).astype(np.uint8))
        hap["rlen"] = hap["ref_len"].copy()
        cl = K.simple_cluster(K.Hap(hap["pos"], hap["rlen"], hap["type"], hap["ref_len"], hap["alt_len"]), 0, gap, 10)
        out.append((hap, cl, v.ctg_seq[v.ctg_off[c]:v.ctg_off[c + 1]].copy()))
    return out


def run_all(params, **kw):
    """vrl_realign over every contig of the callset, each checked against the model -> summed info fields, statuses"""
    from vcfdist_amd import api
    pen = {k: kw[k] for k in ("sub", "open", "extend", "max_qual") if k in kw}
    tot, sts = {}, []
    for hap, cl, seq in callsets(params):
        cols, status, info = check(api.realign(hap, cl, seq, **kw), hap, cl, seq, pen.get("sub", 5), pen.get("open", 6), pen.get("extend", 2),
                                   pen.get("max_qual", 60))
        for f, _ in info._fields_:
            tot[f] = tot.get(f, 0) + getattr(info, f)
        sts.append((hap, cl, status))
    return tot, sts


def check(got, hap, cl, seq, x=5, o=6, e=2, max_qual=60):
    cols, status, info = got
    keep = np.where(status & RM.ST_LIMIT, RM.ST_LIMIT, 0)
    want, want_st = RM.realign(seq, hap, cl.var_beg, x, o, e, max_qual, keep=keep)
    assert (status & ~np.uint8(RM.ST_LIMIT)).tolist() == (want_st & ~np.uint8(RM.ST_LIMIT)).tolist()
    recs = RM.records(cols)
    assert len(recs) == len(want), (len(recs), len(want))
    for k, (a, b) in enumerate(zip(recs, want)):
        for f in ("pos", "rlen", "type", "ref", "alt", "phase_set", "orig_gt"):
            assert a[f] == b[f], (k, f, a, b)
        for f in ("var_qual", "gt_qual"):
            assert np.float32(a[f]).view(np.uint32) == np.float32(b[f]).view(np.uint32), (k, f, a, b)
    assert info.n_clusters == cl.n and info.n_kept == int(np.count_nonzero(status))
    assert info.n_limit == int(np.count_nonzero(status & RM.ST_LIMIT))
    return cols, status, info


@pytest.mark.parametrize("shape", ["wgs", "joint"])
def test_realign_equals_the_model(shape):
    tot, sts = run_all(WGS if shape == "wgs" else JOINT)
    assert tot["n_clusters"] > (2000 if shape == "wgs" else 150), tot["n_clusters"]
    if shape == "joint":      # SV-sized clusters are there
        assert max(max(int(h["ref_len"].max()), int(h["alt_len"].max())) for h, _, _ in sts) >= 50
    assert tot["n_limit"] == 0 and tot["n_realigned"] > 0 and tot["n_rounds"] >= 1


def test_other_penalties_and_many_rounds():
    run_all(JOINT, sub=3, open=2, extend=1, max_qual=40)
    tot, _ = run_all(JOINT, round_bytes=1 << 16)
    assert tot["n_rounds"] > len(callsets(JOINT)) and tot["n_hist_rounds"] > tot["n_rounds"]


def test_job_limit_keeps_the_sv_clusters_original():
    tot, sts = run_all(JOINT, job_bytes_limit=1 << 20)
    assert tot["n_limit"] > 0 and tot["n_kept"] >= tot["n_limit"]
    # the limited clusters are the large ones: every one spans at least 50 bases of reference or haplotype
    for hap, cl, status in sts:
        for c in np.nonzero(status & RM.ST_LIMIT)[0]:
            b, e = cl.var_beg[c], cl.var_beg[c + 1]
            span = hap["pos"][e - 1] + hap["rlen"][e - 1] - hap["pos"][b]
            assert span >= 50 or int(hap["alt_len"][b:e].sum()) >= 50


def test_two_calls_give_identical_output():
    from vcfdist_amd import api
    for hap, cl, seq in callsets(JOINT):
        a, b = api.realign(hap, cl, seq), api.realign(hap, cl, seq)
        for k in a[0]:
            assert np.array_equal(a[0][k], b[0][k]), k
        assert np.array_equal(a[1], b[1])


def test_zero_penalties_are_refused():
    from vcfdist_amd import api
    hap, cl, seq = callsets(dict(WGS, n_sc=50))[0]
    for kw in (dict(sub=0), dict(extend=0)):
        with pytest.raises(api.VprError, match=r"\(-1\)"):
            api.realign(hap, cl, seq, **kw)


# ---- the command lines on the demo files

def _surrogate(tmp_path):
    import demo_pipeline as D
    fa = tmp_path / "surrogate.fa"
    seq = D.surrogate_fasta(5_100_000)
    with open(fa, "w") as fh:
        fh.write(">chr1 surrogate\n")
        s = bytes(seq).decode()
        for i in range(0, len(s), 100000):
            fh.write(s[i:i + 100000] + "\n")
    return str(fa)


def _params(text):
    return [l for l in text.split("\n") if not l.startswith(("out_prefix", "command"))]


def test_command_lines_on_demo_files(tmp_path):
    import demo_pipeline as D
    from vcfdist_amd import cluster as K, io as IO
    fa = _surrogate(tmp_path)
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli = os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")
    rd = lambda p: open(p, "rb").read()
    runs = {}
    for name, cmd in (("c", [cli]), ("py", [sys.executable, "-m", "vcfdist_amd"])):
        for tag, flags in (("ro", ["-rq", "-rt", "-ro"]), ("rq", ["-rq"]), ("only", ["-ro"])):
            pre = str(tmp_path / f"{name}-{tag}") + "/"
            os.makedirs(pre)
            r = subprocess.run(cmd + inputs + ["-p", pre] + flags, capture_output=True, text=True, cwd=ROOT, timeout=1200)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[name, tag] = (pre, r.stdout)
    vcfs = ("orig-query.vcf", "orig-truth.vcf", "query.vcf", "truth.vcf")
    for name in ("c", "py"):
        pre = runs[name, "ro"][0]
        assert sorted(os.listdir(pre)) == sorted(vcfs + ("parameters.txt",))
        par = rd(pre + "parameters.txt").decode()
        assert "realign_truth = true\nrealign_query = true\nrealign_only = true\n" in par
        assert sorted(os.listdir(runs[name, "only"][0])) == ["parameters.txt"]
        assert "realign_truth = false\nrealign_query = false\nrealign_only = true\n" in rd(runs[name, "only"][0] + "parameters.txt").decode()
        assert "realign_query = true\nrealign_only = false\n" in rd(runs[name, "rq"][0] + "parameters.txt").decode()
        assert runs[name, "ro"][1] == "" and "PRECISION-RECALL SUMMARY" in runs[name, "rq"][1]
    for tag in ("ro", "rq", "only"):
        a, b = runs["c", tag][0], runs["py", tag][0]
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)), tag
        for f in os.listdir(a):
            if f == "parameters.txt":
                assert _params(rd(a + f).decode()) == _params(rd(b + f).decode()), (tag, f)
            elif f == "summary.vcf":        # the ##fileDate / ##CL lines differ (the command and its prefix)
                keep = lambda t: [l for l in t.split(b"\n") if not l.startswith((b"##fileDate", b"##CL"))]
                assert keep(rd(a + f)) == keep(rd(b + f)), (tag, f)
            else:
                assert rd(a + f) == rd(b + f), (tag, f)
    assert runs["c", "rq"][1] == runs["py", "rq"][1]
    assert "query.vcf" in os.listdir(runs["c", "rq"][0]) and "truth.vcf" not in os.listdir(runs["c", "rq"][0])
    assert rd(runs["c", "rq"][0] + "query.vcf") == rd(runs["c", "ro"][0] + "query.vcf")
    # query.vcf against the model: the demo query as read, biWFA clusters, the model's realignment and writer
    bed = IO.Bed(os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed"))
    q = IO.read_vcf(os.path.join(D.DEMO, "query.vcf"), bed)
    fasta = IO.read_fasta(fa)
    ctgs = []
    for k, ctg in enumerate(q["contigs"]):
        seq = fasta[ctg]
        haps = []
        for s in q["vars"][k]:
            h = K.HapSeq.__new__(K.HapSeq)
            K.Hap.__init__(h, s["pos"], s["rlen"], s["type"], s["ref_len"], s["alt_len"])
            h.ref_off, h.alt_off, h.pool = s["ref_off"], s["alt_off"], s["pool"]
            cl = K.wfa_cluster(h, bytes(seq), sub=5, open=6, extend=2, max_cluster_itrs=4, reach_min_gap=10)[0]
            haps.append(RM.realign(seq, s, cl.var_beg)[0])
        ctgs.append((ctg, q["lengths"][k], q["ploidy"][k], haps))
    got = rd(runs["c", "ro"][0] + "query.vcf").decode()
    day = got.split("\n")[1][len("##fileDate="):]
    assert day in (datetime.date.today().strftime("%Y%m%d"), (datetime.date.today() - datetime.timedelta(days=1)).strftime("%Y%m%d"))
    assert got == RM.write_vcf(ctgs, q["sample"], fasta, day)
