"""Derived strata on the GPU (include/vcfdist_derive.h, pr_derive.hip): k_derive_mask against the postfix model of
tests/derive_model.py on uploaded words -- slots of 0, 1, 65 and 300 variants, every placement of the new strata against the 64-bit
words, programs to a stack of 32, operands in the word being assembled, in an earlier output word and alternating between two old
words --, the refusals, and both command lines with --stratify-derive / --stratify-cross on one and on two ranks."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library opens the GPU: its HIP runtime is then the process's only one (as tests/test_distributed.py)

import derive_cases as DC
import derive_model as DM
from vcfdist_amd import _abi as A
from vcfdist_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VAR = (0, 1, 65, 300)
AND, OR, NOT = DM.AND, DM.OR, DM.NOT


# ---- 1. the kernel on uploaded words

def old_words(n_prev, seed):
    """random old strata per slot: (member[n_prev][n_var], their words with random bits ABOVE n_prev in the last word -- what a
    read-modify-write without its mask would keep)"""
    rng = np.random.RandomState(seed)
    mem = [DC.random_members(n_prev, n, seed + 7 * s) for s, n in enumerate(N_VAR)]
    words = [DM.words_of(m) for m in mem]
    if n_prev & 63:
        for w in words:
            junk = rng.randint(0, 1 << 62, size=w.shape[1]).astype(np.uint64) * np.uint64(4) + rng.randint(0, 4, size=w.shape[1]).astype(np.uint64)
            w[-1] |= junk << np.uint64(n_prev & 63)
    return mem, words


def programs(n_prev, n_entries, seed):
    """n_entries valid programs: random ones with operands among the old strata and the entries in front, and at fixed places an
    entry that names its immediate predecessor, one whose operands alternate between two old words, one that reaches a stack of
    32, and one in the last output word that names the first entry (an earlier output word when the call spans two)"""
    rng = np.random.RandomState(seed)
    entries = []
    for j in range(n_entries):
        front = n_prev + j
        if j == 1:
            code = [front - 1, NOT, front - 1, OR, front - 1, AND]            # the predecessor, from the register: !p | p & p == p
        elif j == 2 and n_prev > 64:
            lo, hi = rng.randint(0, 64, 6), rng.randint(64, n_prev, 6)       # two old words in turn: the one-word cache misses every time
            code = [int(lo[0])]
            for a, b in zip(hi, lo[1:].tolist() + [int(lo[0])]):
                code += [int(a), (AND, OR)[rng.randint(2)], int(b), (AND, OR)[rng.randint(2)]]
        elif j == 3 or (j == 0 and n_entries == 1 and n_prev > 1):
            code = DC.deep_program(rng, front, 32)
        elif j == n_entries - 1 and j > 3:
            code = [n_prev, int(rng.randint(front)), OR, n_prev + 1, NOT, AND]    # the first entries, read back from the lane's own store
        else:
            code = DC.random_program(rng, front)
        entries.append(code)
    return entries


def flat(entries):
    off = np.cumsum([0] + [len(e) for e in entries]).astype(np.int32)
    return off, np.asarray([c for e in entries for c in e], np.int32)


def check(got, mem_old, words_old, entries, n_prev):
    n_new = n_prev + len(entries)
    off, code = flat(entries)
    for s, n in enumerate(N_VAR):
        assert got[s].shape == ((n_new + 63) // 64, n), (s, got[s].shape)
        want = DM.run_programs(off, code, mem_old[s])
        bits = DM.bits_of(got[s], n_new)
        assert np.array_equal(bits[:n_prev], mem_old[s]), s                                  # the old bits are unchanged
        full = n_prev >> 6
        assert np.array_equal(got[s][:full], words_old[s][:full]), s                         # ... and so are the full old words
        bad = np.nonzero(bits[n_prev:] != want[n_prev:])
        assert len(bad[0]) == 0, (s, bad[0][:5] + 0, bad[1][:5])                             # the new bits equal the model
        if n_new & 63:
            assert not (got[s][-1] >> np.uint64(n_new & 63)).any(), s                        # nothing at and above n_strata
    return [DM.run_programs(off, code, m) for m in mem_old]


SHAPES = [(1, 1), (63, 1), (63, 2), (64, 1), (60, 10), (5, 64), (127, 130), (130, 1), (3, 200)]


@pytest.mark.parametrize("n_prev,n_entries", SHAPES)
def test_new_bits_equal_the_model(n_prev, n_entries):
    mem, words = old_words(n_prev, 100 * n_prev + n_entries)
    entries = programs(n_prev, n_entries, 31 * n_prev + n_entries)
    off, code = flat(entries)
    pr = api.PrecisionRecall()
    pr.upload_strata_masks(n_prev, words)
    pr.derive_masks(off, code)
    assert pr.derive_timing() > 0
    got = pr.download_strata_masks()
    full = check(got, mem, words, entries, n_prev)
    if n_entries >= 3:
        assert any(m[n_prev:].any() for m in full) and not all(m[n_prev:].all() for m in full)       # the programs are not vacuous
    if (n_prev, n_entries) == (60, 10):      # entry 9 (stratum 69, output word 1) names entries 0 and 1 (output word 0)
        assert entries[9][0] == 60 and entries[9][3] == 61 and 69 >> 6 == 1 and 60 >> 6 == 0
    if n_prev > 64 and n_entries > 2:        # the alternating entry's operands change word at every push
        ops = [c >> 6 for c in entries[2] if c >= 0]
        assert all(a != b for a, b in zip(ops, ops[1:])) and len(ops) == 13
    # two runs agree
    pr.upload_strata_masks(n_prev, words)
    pr.derive_masks(off, code)
    again = pr.download_strata_masks()
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    # a second call on top of the first gives the bits of one call with both entry sets
    if n_entries >= 2:
        cut = n_entries // 2
        pr.upload_strata_masks(n_prev, words)
        pr.derive_masks(*flat(entries[:cut]))
        pr.derive_masks(*flat(entries[cut:]))
        twice = pr.download_strata_masks()
        assert all(np.array_equal(a, b) for a, b in zip(got, twice))


def test_refusals_leave_the_words_as_they_were():
    pr = api.PrecisionRecall()

    def refused(code_rc, off, code):
        with pytest.raises(api.VprError) as e:
            pr.derive_masks(np.asarray(off, np.int32), np.asarray(code, np.int32))
        assert f"({code_rc})" in str(e.value) and "vpr_derive_masks" in str(e.value), str(e.value)
        return str(e.value)
    # no resident words
    assert "no resident membership words" in refused(-4, [0, 1], [0])
    n_prev = 5
    mem, words = old_words(n_prev, 77)
    pr.upload_strata_masks(n_prev, words)
    before = pr.download_strata_masks()
    deep33 = list(range(5)) * 6 + [0, 1, 2] + [AND] * 32
    assert len([c for c in deep33 if c >= 0]) == 33
    assert "entry 0" in refused(-1, [0, len(deep33)], deep33) and "stack exceeds 32" in refused(-1, [0, len(deep33)], deep33)
    deep32 = deep33[1:33] + [AND] * 31
    assert "underflows" in refused(-1, [0, 2], [0, AND]) and "underflows" in refused(-1, [0, 1], [NOT]) and "underflows" in refused(-1, [0, 3], [0, 1, OR][::-1])
    assert "entry 1" in refused(-1, [0, 1, 3], [0, 0, AND])                                   # (the second entry underflows)
    assert "ends at depth 2" in refused(-1, [0, 2], [0, 1])                                   # a leftover stack
    assert "ends at depth 0" in refused(-1, [0, 0], [0])                                      # an empty program
    assert "operand 5" in refused(-1, [0, 1], [5])                                            # its own index
    assert "entry 1" in refused(-1, [0, 1, 2], [4, 6]) and "operand 6" in refused(-1, [0, 1, 2], [4, 6])
    assert "operand 7" in refused(-1, [0, 1], [7])
    assert "unknown opcode -4" in refused(-1, [0, 2], [0, -4])
    assert "n_entries 0" in refused(-1, [0], [0])
    assert "n_entries 1025" in refused(-1, list(range(1026)), [0] * 1025)
    assert "exceeds 65536" in refused(-1, [0, 65537], [0] + [NOT] * 65536)                    # code above the cap
    assert "decreases" in refused(-1, [0, 2, 1], [0, NOT])
    after = pr.download_strata_masks()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))                           # the words are still valid, and the same
    # the limits themselves are accepted, and after the refusals the handle still makes the right words
    entries = [deep32, [0] + [NOT] * 65000]
    pr.derive_masks(*flat(entries))
    check(pr.download_strata_masks(), mem, words, entries, n_prev)
    pr.derive_masks(*flat([[k % 7] for k in range(1024)]))                                    # 1024 entries in one call
    got = pr.download_strata_masks()
    assert got[3].shape == ((7 + 1024 + 63) // 64, 300)
    bits = DM.bits_of(got[3], 7 + 1024)
    assert all(np.array_equal(bits[7 + k], bits[k % 7]) for k in range(1024))


# ---- 2. the command lines

OTHERS = ["--stratify-context", "--stratify-variants"]
# (the demo's surrogate FASTA is random: its homopolymers are short, hp_4to6 is the homopolymer stratum with members)
ENTRIES = ["same=hp_4to6", "easy=!*", "any=*", "dm=!(hp_4to6|snp_ti)", "dm2=!hp_4to6&!snp_ti", "nothp=!hp_4to6", "nohom=!hom",
           "easy_ctx=!(hp_*|tr_*|gc_*)", "d_hp=del_1to5 & (hp_4to6 | hp_7to11)"]
CROSS = ["ins_*,del_*:hp_*", "same:het"]
FULL = ["--bootstrap", "20", "--classify-errors", "--cut-classes"]
DV_FILE = "derived-strata.tsv"


def derive_options():
    return [a for e in ENTRIES for a in ("--stratify-derive", e)] + [a for e in CROSS for a in ("--stratify-cross", e)]


def _write_fasta(path, seq, contigs):
    s = bytes(seq).decode()
    with open(path, "w") as fh:
        for c in contigs:
            fh.write(f">{c}\n")
            for i in range(0, len(s), 100000):
                fh.write(s[i:i + 100000] + "\n")
    return str(path)


def _without_command(path):
    """a file's bytes without the lines that record the command line, the output prefix or the date"""
    return b"\n".join(l for l in open(path, "rb").read().split(b"\n") if not l.startswith((b"##fileDate", b"##CL=", b"command = ", b"out_prefix = ")))


def rows_of(path, stratum=None):
    """the rows of a table with a STRATUM (or NAME) column in front: {stratum: [the rest of each row]}, or one stratum's list"""
    out = {}
    for l in open(path).read().split("\n")[1:-1]:
        name, rest = l.split("\t", 1)
        out.setdefault(name, []).append(rest)
    return out if stratum is None else out[stratum]


@pytest.fixture(scope="module")
def demo_runs(tmp_path_factory):
    """the demo callsets through both command lines: without the options, with them (both drivers), and two runs without files"""
    import demo_pipeline as D
    tmp = tmp_path_factory.mktemp("derive_demo")
    fa = _write_fasta(tmp / "surrogate.fa", D.surrogate_fasta(5_100_000), ("chr1",))
    inputs = [os.path.join(D.DEMO, "query.vcf"), os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.vcf.gz"), fa,
              "-b", os.path.join(D.DEMO, "nist-v4.2.1_chr1_5Mb.bed")]
    cli, py = [os.path.join(ROOT, "vcfdist_amd", "lib", "vcfdist_gpu")], [sys.executable, "-m", "vcfdist_amd"]
    runs = {}
    for name, cmd, extra in (("c-off", cli, OTHERS + FULL), ("c-dv", cli, OTHERS + FULL + derive_options()), ("py-dv", py, derive_options() + FULL + OTHERS),
                             ("c-ctx-n", cli, ["-n", "--stratify-context"]),
                             ("c-dv-n", cli, ["-n", "--stratify-context", "--stratify-derive", "easy=!*", "--stratify-cross", "easy:hp_*"])):
        pre = str(tmp / name) + "/"
        os.makedirs(pre)
        r = subprocess.run(cmd + inputs + ["-p", pre] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (pre, r.stdout, r.stderr)
    return runs, inputs


def test_both_drivers_write_the_same_files(demo_runs):
    runs, _ = demo_runs
    c, p = runs["c-dv"][0], runs["py-dv"][0]
    files = sorted(os.listdir(c))
    assert files == sorted(os.listdir(p)) and DV_FILE in files
    for f in files:
        assert _without_command(c + f) == _without_command(p + f), f
    assert runs["c-dv"][1] == runs["py-dv"][1] == runs["c-off"][1]
    # the table order: the families' strata, the derived entries in command-line order, the crossed pairs option by option
    order = [l.split("\t", 1)[0] for l in open(c + "stratified-precision-recall-summary.tsv").read().split("\n")[1:-1]]
    order = [n for i, n in enumerate(order) if i == 0 or order[i - 1] != n]
    pairs = [f"{a}&{b}" for a in DC.VARIANT[2:10] for b in DC.CONTEXT[:3]] + ["same&het"]
    assert order == DC.NAMES + [e.split("=")[0] for e in ENTRIES] + pairs
    text = open(c + DV_FILE).read().split("\n")
    assert text[0] == "NAME\tKIND\tEXPRESSION\tQUERY_MEMBERS\tTRUTH_MEMBERS" and text[-1] == "" and len(text) == 2 + len(ENTRIES) + 25
    assert [l.split("\t")[:3] for l in text[1:-1]] == [[e.split("=")[0], "derive", e.split("=", 1)[1]] for e in ENTRIES] + [[n, "cross", n] for n in pairs]
    for name in ("c-dv", "py-dv"):
        m = re.findall(r"derived strata: (\d+) strata \((\d+) derived, (\d+) crossed\), ([0-9.]+) ms on the device", runs[name][2])
        assert len(m) == 1 and [int(x) for x in m[0][:3]] == [len(ENTRIES) + 25, len(ENTRIES), 25] and float(m[0][3]) > 0, runs[name][2][-600:]


def test_without_the_options_nothing_changes(demo_runs):
    runs, _ = demo_runs
    off, on = runs["c-off"][0], runs["c-dv"][0]
    plain = sorted(os.listdir(off))
    assert DV_FILE not in plain and sorted(set(os.listdir(on)) - {DV_FILE}) == plain
    assert "derived strata" not in runs["c-off"][2] and "derived strata" not in runs["c-ctx-n"][2]
    n_lines = lambda err: len([l for l in err.split("\n") if l.startswith("[vcfdist_amd]")])
    assert n_lines(runs["c-dv"][2]) == n_lines(runs["c-off"][2]) + 1                         # one more stderr line
    for f in plain:
        a, b = _without_command(off + f), _without_command(on + f)
        if f.startswith("stratified-"):              # the old strata's rows are the old rows, in front of the new ones
            la, lb = a.split(b"\n")[:-1], b.split(b"\n")[:-1]
            assert lb[:len(la)] == la and len(lb) > len(la), f
        else:
            assert a == b, f
    # -n: no file appears, the line is there
    assert os.listdir(runs["c-dv-n"][0]) == [] and os.listdir(runs["c-ctx-n"][0]) == []
    assert re.search(r"derived strata: 4 strata \(1 derived, 3 crossed\), [0-9.]+ ms on the device", runs["c-dv-n"][2])


def test_same_partition_and_de_morgan(demo_runs):
    runs, _ = demo_runs
    c = runs["c-dv"][0]
    tables = [f for f in sorted(os.listdir(c)) if f.startswith("stratified-")]
    assert tables == ["stratified-bootstrap-precision-recall-summary.tsv", "stratified-error-classes-summary.tsv", "stratified-error-classes.tsv",
                      "stratified-precision-recall-summary.tsv", "stratified-precision-recall.tsv"]
    for f in tables:        # the derived strata appear in every stratified table; same is hp_4to6 and dm is dm2, but for the name
        rows = rows_of(c + f)
        assert rows["same"] == rows["hp_4to6"] and len(rows["same"]) >= 4, f
        assert rows["dm"] == rows["dm2"] and rows["dm"] != rows["nothp"], f
        assert len(rows["same&het"]) == len(rows["same"]), f                                 # (a cross names a derived stratum)
    # x plus !x is precision-recall.tsv in every cell that counts, for a BED-like stratum and for a variant stratum
    total = [l.split("\t") for l in open(c + "precision-recall.tsv").read().split("\n")[1:-1]]
    rows = rows_of(c + "stratified-precision-recall.tsv")
    for x, not_x in (("hp_4to6", "nothp"), ("hom", "nohom"), ("any", "easy")):
        a, b = ([r.split("\t") for r in rows[n]] for n in (x, not_x))
        assert len(a) == len(b) == len(total) > 100
        n_cells = 0
        for ra, rb, rt in zip(a, b, total):
            assert ra[:2] == rb[:2] == rt[:2]
            for col in range(6, 12):
                assert int(ra[col]) + int(rb[col]) == int(rt[col]), (x, ra[:2], col)
                n_cells += int(rt[col]) > 0
        assert n_cells > 100
    assert any(int(r.split("\t")[6]) > 0 for r in rows["nothp"]) and any(int(r.split("\t")[6]) > 0 for r in rows["hp_4to6"])


def test_easy_is_the_count_of_the_stderr_line(demo_runs):
    runs, _ = demo_runs
    members = {name: (int(q), int(t)) for name, (_, _, q, t) in ((n, r[0].split("\t")) for n, r in rows_of(runs["c-dv"][0] + DV_FILE).items())}
    none = lambda err: [int(x) for x in re.findall(r"stratified: \d+ strata, (\d+) of (\d+) hap-variants in none of them", err)[0]]
    # in none of the context and variant strata: the count of the run without the options
    n_none, n_all = none(runs["c-off"][2])
    assert sum(members["easy"]) == n_none and sum(members["any"]) == n_all - n_none
    # in none of the context strata: the count of the run with the context strata alone
    n_none_ctx, n_all_ctx = none(runs["c-ctx-n"][2])
    assert n_all_ctx == n_all and sum(members["easy_ctx"]) == n_none_ctx and 0 < n_none_ctx < n_all
    assert none(runs["c-dv"][2]) == [0, n_all] and none(runs["c-dv-n"][2]) == [0, n_all]    # (easy or any: never none)
    assert members["dm"] == members["dm2"] and members["same&het"][0] <= members["same"][0]
    assert sum(members["same"]) + sum(members["nothp"]) == n_all and sum(members["same"]) > 100


def test_member_counts_equal_the_model_on_downloaded_words(demo_runs):
    """the demo contig prepared as the Python driver prepares it, the context and variant words made and downloaded, then the model
    on those bits against derived-strata.tsv and against vpr_derive_masks' own words"""
    from vcfdist_amd import __main__ as CLI
    runs, inputs = demo_runs
    args = CLI.parse(inputs + OTHERS + derive_options())
    plan = CLI.plan_strata(args)
    inp = CLI.read_inputs(args, inputs)
    assert inp.contigs == ["chr1"]
    prep = CLI.prepare_contig("chr1", inp.fasta["chr1"], inp.slots_of("chr1"), args)
    pr = api.PrecisionRecall()
    pr.context_masks(prep["variants"], plan.ctx.specs)
    pr.varstrata_masks(prep["variants"], plan.vs.specs, append=True)
    base = pr.download_strata_masks()
    pr.derive_masks(plan.derived.code_off, plan.derived.code)
    got = pr.download_strata_masks()
    q, t = np.zeros(len(plan.derived.names), np.int64), np.zeros(len(plan.derived.names), np.int64)
    for s in range(4):
        mem = DM.bits_of(base[s], 25)
        names, full = DM.derive(ENTRIES, DC.NAMES, mem)
        names, full = DM.cross(CROSS, names, full)
        assert names == plan.names
        assert np.array_equal(DM.bits_of(got[s], len(names)), full), s
        (q if s < 2 else t)[:] += full[25:].sum(axis=1)
    rows = rows_of(runs["c-dv"][0] + DV_FILE)
    assert [(int(r[0].split("\t")[2]), int(r[0].split("\t")[3])) for r in rows.values()] == list(zip(q.tolist(), t.tolist()))
    assert list(rows) == plan.derived.names and q.sum() > 1000 and (q[2:] > 0).sum() > 10


@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """the demo callsets twice, as chr1 and chr2 (the inputs of tests/test_gpu_varstrata.py's two-rank test), and the one-rank run with
    the context and variant strata, derived and crossed strata, a bootstrap and the error classes cut by all of them"""
    import gzip
    import demo_pipeline as D
    tmp = tmp_path_factory.mktemp("derive_two")
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
    base = [str(qv), str(tv), fa, "-b", str(bed)] + OTHERS + derive_options() + ["--bootstrap", "8", "--classify-errors", "--cut-classes"]
    (tmp / "one").mkdir()
    subprocess.run([sys.executable, "-m", "vcfdist_amd"] + base + ["-p", str(tmp / "one") + "/"], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL, timeout=600)
    return tmp, base, env


@pytest.mark.parametrize("how", ["superclusters", "contigs"])
def test_command_line_two_ranks(two_contigs, demo_runs, how):
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
    files = sorted(os.listdir(tmp / "one"))
    assert DV_FILE in files and sorted(os.listdir(out)) == files
    for name in files:
        if name.startswith(("stratified-", "precision-recall", "bootstrap-", "error-classes")) or name in (DV_FILE, "variant-strata.tsv"):
            one, two = (tmp / "one" / name).read_bytes(), (out / name).read_bytes()
            assert one == two and len(one) > 60, name
    # both contigs hold the demo callsets: every derived stratum has twice the demo's members
    demo = rows_of(demo_runs[0]["c-dv"][0] + DV_FILE)
    for name, r in rows_of(str(out / DV_FILE)).items():
        d, g = demo[name][0].split("\t"), r[0].split("\t")
        assert g[:2] == d[:2] and [int(g[2]), int(g[3])] == [2 * int(d[2]), 2 * int(d[3])], name
