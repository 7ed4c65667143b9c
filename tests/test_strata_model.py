"""Host side of the region-stratified counters (include/vcfdist_strata.h): the exported symbols, the BED interval accessor,
the strata list reader, the stratified writer and the command line's option.  No GPU."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import strata_model as M
from vcfdist_amd import api, io as IO, report as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported():
    text = open(os.path.join(ROOT, "include", "vcfdist_strata.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint\s+(vpr_\w+)\s*\(", text)
    assert {"vpr_strata_masks", "vpr_strata_download_masks", "vpr_strata_upload_masks", "vpr_pr_counts_strata",
            "vpr_allreduce_counts_strata"} <= set(names)
    assert sorted(names) == sorted(api.STRATA_EXPORTED)
    L = api.lib()
    for n in names + ["vio_bed_intervals", "vrp_write_stratified"]:
        assert hasattr(L, n), n
    assert "vio_bed_intervals" in IO.EXPORTED and "vrp_write_stratified" in RP.EXPORTED


@pytest.mark.parametrize("gz", [False, True])
def test_bed_intervals_return_what_was_read(tmp_path, gz):
    rows = [("chr2", 5, 9), ("chr1", 10, 20), ("chr1", 20, 30), ("chr1", 40, 50), ("chr2", 9, 100)]
    text = "".join(f"{c}\t{a}\t{b}\n" for c, a, b in rows)
    p = str(tmp_path / ("r.bed.gz" if gz else "r.bed"))
    with (gzip.open(p, "wt") if gz else open(p, "w")) as fh:
        fh.write(text)
    bed = IO.Bed(p)
    st, sp = bed.intervals("chr1")
    assert st.dtype == np.int32 and st.tolist() == [10, 20, 40] and sp.tolist() == [20, 30, 50]
    st, sp = bed.intervals("chr2")
    assert st.tolist() == [5, 9] and sp.tolist() == [9, 100]
    st, sp = bed.intervals("chr3")
    assert len(st) == 0 and len(sp) == 0
    # the host loop over many variants is vio_bed_contains, one call after the other
    pos = np.array([9, 10, 19, 20, 25, 30, 49, 50, 18], np.int32)
    rl = np.array([1, 1, 0, 0, 20, 10, 0, 1, 4], np.int32)
    ty = np.array([1, 1, 2, 2, 3, 3, 2, 1, 3], np.uint8)
    many = bed.contains_many("chr1", pos, rl, ty)
    assert many.tolist() == [bed.contains("chr1", int(p), int(p + r), int(t)) for p, r, t in zip(pos, rl, ty)]
    assert set(many.tolist()) == {0, 1, 2} and set(bed.contains_many("chr3", pos, rl, ty).tolist()) == {3}
    s = IO.contig_strata([bed], ["chr2", "chrX", "chr1"])
    assert (s.n_strata, s.n_ctg) == (1, 3) and s.iv_off.tolist() == [0, 2, 2, 5]
    assert s.iv_start.tolist() == [5, 9, 10, 20, 40] and s.iv_stop.tolist() == [9, 100, 20, 30, 50]


def test_read_strata_resolves_paths_and_refuses_bad_lists(tmp_path):
    sub = tmp_path / "lists"
    (sub / "beds").mkdir(parents=True)
    M.write_bed(sub / "beds" / "a.bed", [("chr1", 0, 10)])
    M.write_bed(tmp_path / "abs.bed", [("chr1", 5, 6), ("chr1", 6, 8)])
    lst = sub / "strata.tsv"
    lst.write_text(f"# comment\n\nrel\tbeds/a.bed\nabs\t{tmp_path / 'abs.bed'}\n")
    cwd = os.getcwd()
    os.chdir(str(tmp_path))           # relative paths resolve against the list's directory, not the working directory
    try:
        names, beds = IO.read_strata(os.path.join("lists", "strata.tsv"))
    finally:
        os.chdir(cwd)
    assert names == ["rel", "abs"]
    assert beds[0].intervals("chr1")[1].tolist() == [10] and beds[1].intervals("chr1")[0].tolist() == [5, 6]

    def refused(text, what, beds=()):
        for name, rows in beds:
            M.write_bed(sub / name, rows)
        lst.write_text(text)
        with pytest.raises(IOError) as e:
            IO.read_strata(str(lst))
        assert re.search(what, str(e.value)), str(e.value)
    refused("x\tbeds/a.bed\nx\tbeds/a.bed\n", "duplicate stratum name 'x'")
    refused("x\tbeds/missing.bed\n", "stratum 'x'.*Failed to open")
    refused("x\tu.bed\n", "stratum 'x'.*unsorted", [("u.bed", [("chr1", 50, 60), ("chr1", 10, 20)])])
    refused("x\to.bed\n", "stratum 'x'.*overlap", [("o.bed", [("chr1", 10, 20), ("chr1", 19, 30)])])
    refused("x\tz.bed\n", "stratum 'x'.*length zero", [("z.bed", [("chr1", 10, 10)])])
    refused("x\tr.bed\n", "stratum 'x'.*stop precedes start", [("r.bed", [("chr1", 10, 5)])])
    (sub / "m.bed").write_text("chr1\t10\n")
    refused("x\tm.bed\n", "stratum 'x'.*fewer than 3 fields")
    refused("just-a-name\n", "expected name<TAB>path")
    refused("# nothing\n\n", "names no stratum")
    with pytest.raises(IOError):
        IO.read_strata(str(sub / "no-such-list.tsv"))


def test_stratified_writer_rows_equal_the_unstratified_writer(tmp_path):
    rng = np.random.RandomState(11)
    names = ["whole genome", "lowmap", "empty"]
    for min_qual, max_qual in ((0, 60), (10, 40)):
        nq = max_qual - min_qual + 1
        counts = np.zeros((3, 2, 4, 3, nq), np.int64)
        for k in range(2):          # monotone counters like the real ones; stratum 2 stays all zero
            for cs in range(2):
                for t in range(3):
                    for e in range(3):
                        counts[k, cs, t, e] = np.sort(rng.randint(0, 5000 >> (4 * k), size=nq))[::-1]
                counts[k, cs, 3] = counts[k, cs, :3].sum(axis=0)
        pre = str(tmp_path / f"q{min_qual}") + "/"
        os.makedirs(pre)
        RP.write_stratified(pre, names, counts, min_qual, max_qual)
        for k in range(3):
            os.makedirs(str(tmp_path / f"q{min_qual}_{k}"))
            RP.write_precision_recall(str(tmp_path / f"q{min_qual}_{k}") + "/", counts[k], min_qual, max_qual)
        for strat, plain, header in (("stratified-precision-recall.tsv", "precision-recall.tsv", "STRATUM\tVAR_TYPE\tMIN_QUAL\tPREC\t"),
                                     ("stratified-precision-recall-summary.tsv", "precision-recall-summary.tsv",
                                      "STRATUM\tVAR_TYPE\tTHRESHOLD\tMIN_QUAL\t")):
            lines = open(pre + strat).read().split("\n")
            assert lines[0].startswith(header) and lines[-1] == ""
            body = lines[1:-1]
            per = len(body) // 3
            assert [l.split("\t", 1)[0] for l in body] == [n for n in names for _ in range(per)]      # strata in list order
            for k, n in enumerate(names):
                want = open(str(tmp_path / f"q{min_qual}_{k}" / plain), "rb").read()
                got = "".join(l.split("\t", 1)[1] + "\n" for l in lines[:1] + body[k * per:(k + 1) * per]).encode()
                assert got == want, (strat, n)
    with pytest.raises(RP.ReportError):
        RP.write_stratified(str(tmp_path) + "/", ["one"], np.zeros((2, 2, 4, 3, 61), np.int64), 0, 60)


def test_command_line_help_names_the_option():
    r = subprocess.run([sys.executable, "-m", "vcfdist_amd", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--stratify" in r.stdout
