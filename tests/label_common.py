"""What the GPU tests of the two label passes (tests/test_gpu_errclass.py, tests/test_gpu_matchkind.py) share: the variant classes of
a batch and the pieces of their command-line tests."""
import gzip
import os
import subprocess
import sys

from vcfdist_amd import summary as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def var_classes(v, sv_threshold=50):
    return [S.var_class(v.var_type[s], v.var_ref_len[s], v.var_alt_len[s], sv_threshold) for s in range(4)]


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


def two_contig_run(tmp, options):
    """the demo callsets twice, as chr1 and chr2 (the inputs of tests/test_gpu_varstrata.py's two-rank test), written under tmp, and
    the one-rank run with `options` into tmp/one -> (tmp, the command line's arguments without the prefix, the environment)"""
    import demo_pipeline as D
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
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), VCFDIST_ONE_GPU="1")
    base = [str(qv), str(tv), fa, "-b", str(bed)] + options
    (tmp / "one").mkdir()
    subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL, timeout=660)
    return tmp, base, env
