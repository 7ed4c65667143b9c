"""The numpy model of the sequence-context strata (tests/context_model.py) on hand cases, the C ABI's declarations, and the
conditions the GPU tests' inputs (tests/context_cases.py) have to meet for those tests not to pass vacuously."""
import os
import re

import numpy as np
import pytest

import context_cases as CC
import context_model as CM
import strata_model as M
from vcfdist_amd import _abi as A
from vcfdist_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def iv(s, spec):
    return [(int(a), int(b)) for a, b in zip(*CM.intervals(s, spec))]


def test_header_and_library_agree():
    text = open(os.path.join(ROOT, "include", "vcfdist_context.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bint\s+(vpr_\w+)\s*\(", code)
    assert sorted(names) == sorted(api.CONTEXT_EXPORTED) and len(names) == 6
    L = api.lib()
    for n in names + ["vrp_write_context_bed"]:
        assert hasattr(L, n), n
    fields = re.search(r"typedef struct vpr_context_stratum \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f for f, _ in A.VprContextStratum._fields_]
    assert (int(re.search(r"#define VPR_CTX_PERIOD (\d+)", text).group(1)), int(re.search(r"#define VPR_CTX_GC (\d+)", text).group(1))) == \
        (A.CTX_PERIOD, A.CTX_GC)


def test_default_set():
    names, specs = api.context_default()
    assert names == ["hp_4to6", "hp_7to11", "hp_ge12", "tr_di_ge10", "tr_tri_ge14", "tr_quad_ge19",
                     "gc_lt25", "gc_25to30", "gc_30to55", "gc_55to65", "gc_ge65"]
    per = [(s.period, s.min_len, s.max_len, s.slop) for s in specs[:6]]
    assert per == [(1, 4, 6, 5), (1, 7, 11, 5), (1, 12, 0, 5), (2, 10, 0, 5), (3, 14, 0, 5), (4, 19, 0, 5)]
    assert all(s.kind == A.CTX_PERIOD for s in specs[:6]) and all(s.kind == A.CTX_GC for s in specs[6:])
    assert [(s.gc_lo, s.gc_hi, s.window, s.slop) for s in specs[6:]] == [(0, 25, 100, 0), (25, 30, 100, 0), (30, 55, 100, 0),
                                                                        (55, 65, 100, 0), (65, 101, 100, 0)]
    assert api.context_info() == (4096, 16)


def test_model_period_hand_cases():
    s = "AAAACGTNNAAAAACACACACACGTTTT"
    assert iv(s, A.ctx_period(1, 4)) == [(0, 4), (9, 14), (24, 28)]
    assert iv(s, A.ctx_period(2, 6)) == [(13, 23)]
    assert iv("GGACACACACACTT", A.ctx_period(4, 9)) == []                   # ACAC... has period 2: not a period-4 tract
    assert iv("GGACACACACACTT", A.ctx_period(2, 5)) == [(2, 12)]
    assert iv("GGACGTACGTACGTT", A.ctx_period(4, 9)) == [(2, 14)]
    assert iv("GGACGTACGTACGTT", A.ctx_period(4, 5)) == [(0, 14)]           # GGACG is a period-4 tract of five bases: merged with it
    assert iv("TAAAAAAT", A.ctx_period(2, 3)) == [] and iv("TAAAAAAT", A.ctx_period(1, 3)) == [(1, 7)]
    assert iv("ACGACGACG", A.ctx_period(6, 7)) == [] and iv("ACGACGACG", A.ctx_period(3, 7)) == [(0, 9)]
    # lengths around the limits
    for n, want in ((3, []), (4, [(1, 5)]), (6, [(1, 7)]), (7, [])):
        assert iv("C" + "A" * n + "G", A.ctx_period(1, 4, 6)) == want, n
    # an N ends a run, and is no base of one
    assert iv("AAANAAA", A.ctx_period(1, 3)) == [(0, 3), (4, 7)] and iv("NNNNN", A.ctx_period(1, 2)) == []
    # two period-2 tracts that share a base are merged at slop 0; two homopolymers of different bases abut
    assert iv("ACACAGAGAG", A.ctx_period(2, 5)) == [(0, 10)] and iv("ACACAGAGAG", A.ctx_period(2, 6)) == [(4, 10)]
    assert iv("TAAAACCCCT", A.ctx_period(1, 4)) == [(1, 9)]
    # slop: overlap, abut, miss by one; clipped at both ends
    assert iv(CC.PAD_CONTIG, A.ctx_period(1, 4, 0, 2)) == [(0, 21), (22, 29)]
    assert iv(CC.PAD_CONTIG, A.ctx_period(1, 4, 0, 0)) == [(0, 4), (7, 11), (15, 19), (24, 28)]
    assert iv("", A.ctx_period(1, 2)) == [] and iv("A", A.ctx_period(1, 2)) == [] and iv("AA", A.ctx_period(1, 2)) == [(0, 2)]


def test_model_gc_hand_cases():
    assert iv("ATGCA", A.ctx_gc(40, 60, 5)) == [(2, 3)]                      # W odd: the window of base 2 is [0, 5): g = 2
    assert iv("ATGCA", A.ctx_gc(41, 60, 5)) == [] and iv("ATGCA", A.ctx_gc(0, 40, 5)) == []     # 100 g == lo W is in, == hi W is out
    assert iv("ATGC", A.ctx_gc(50, 75, 4)) == [(2, 3)]                       # W even: the window of base 2 is [0, 4)
    assert iv("GTGC", A.ctx_gc(50, 75, 4)) == [] and iv("GTGC", A.ctx_gc(75, 101, 4)) == [(2, 3)]
    assert iv("ATNCATGCA", A.ctx_gc(0, 101, 4)) == [(5, 8)]                  # an N in the window
    assert iv("ACG", A.ctx_gc(0, 101, 4)) == []                              # a contig shorter than W
    assert iv("ACGNT", A.ctx_gc(0, 101, 1)) == [(0, 3), (4, 5)]
    assert iv("GGGGAAAAGGGG", A.ctx_gc(100, 101, 2, 1)) == [(0, 5), (8, 12)]   # flags 1-3 and 9-11, slop 1
    assert iv("GGGGAGGGG", A.ctx_gc(100, 101, 2, 1)) == [(0, 9)]             # [0, 5) and [5, 9) abut


def test_written_beds_are_the_intervals(tmp_path):
    """the helper behind the words / counters / command-line tests: the model's intervals read back through the BED reader"""
    from vcfdist_amd import io as IO
    contigs, specs = CC.hand_case()
    names = [f"c{k}" for k in range(len(contigs))]
    rows = CM.all_intervals(contigs, specs)
    path, strata = CM.write_model_strata(tmp_path, [f"x{k}" for k in range(len(specs))], names, rows)
    got_names, beds = IO.read_strata(path)
    st = M.strata_of(beds, names)
    want = A.Strata(rows, len(contigs))
    assert np.array_equal(st.iv_off, want.iv_off) and np.array_equal(st.iv_start, want.iv_start) and np.array_equal(st.iv_stop, want.iv_stop)
    assert CM.context_bed_text(["p", "q"], ["c0", "c1"], [[([1], [2]), ([], [])], [([0, 5], [3, 9]), ([7], [8])]]) == \
        "c0\t1\t2\tp\nc0\t0\t3\tq\nc0\t5\t9\tq\nc1\t7\t8\tq\n"


# ---- non-vacuity of the GPU tests' inputs

def test_hand_case_is_not_vacuous():
    contigs, specs = CC.hand_case()
    assert all(len(c) <= 200 for c in contigs) and {0, 1} <= {len(c) for c in contigs}
    rows = CM.all_intervals(contigs, specs)
    sizes = [len(rows[k][c][0]) for k in range(len(specs)) for c in range(len(contigs))]
    assert 0 in sizes and max(sizes) > 1
    assert all(any(len(rows[k][c][0]) for c in range(len(contigs))) for k in range(len(specs))), "a stratum without any interval"
    r = lambda k, c: [(int(a), int(b)) for a, b in zip(*rows[k][c])]
    assert r(0, 0)[0][0] == 0 and r(0, 0)[-1][1] == len(contigs[0])           # tracts at the first and the last base
    assert r(1, 5) == [] and r(1, 6) == [] and r(7, 5) == [(0, 6)] and r(7, 6) == [(0, 6)]     # the AAA | AAA seam; W = 1 flags touch it
    assert r(0, 7) == [(10, 16), (32, 36)]                                    # N inside a run, lengths 3, 4, 6, 7 against 4..6
    assert r(1, 8) == [(0, 21), (22, 29)] and r(2, 9) == [(0, 10)] and r(3, 1) == [] and r(3, 2) == [(2, 14)]
    assert r(9, 11) == [] and r(9, 13) == [(25, 40)]                                  # shorter than W; long enough
    # GC: a window with 100 g == lo W (flagged) and one with 100 g == hi W (not flagged), and an N in a window
    s = CM.as_bytes(CC.GC_CONTIG)
    sp = specs[6]
    W, half = sp.window, sp.window // 2
    flag = CM.gc_flags(s, sp.gc_lo, sp.gc_hi, W)
    g = np.array([int(np.isin(s[i - half:i - half + W], [67, 71]).sum()) for i in range(half, len(s) - W + half + 1)])
    clean = np.array([bool(CM.called(s[i - half:i - half + W]).all()) for i in range(half, len(s) - W + half + 1)])
    f = flag[half:len(s) - W + half + 1]
    assert (f[clean & (100 * g == sp.gc_lo * W)]).all() and (clean & (100 * g == sp.gc_lo * W)).any()
    assert not (f[clean & (100 * g == sp.gc_hi * W)]).any() and (clean & (100 * g == sp.gc_hi * W)).any()
    assert (~clean).any() and not f[~clean].any()


def test_seam_case_is_not_vacuous():
    bpw, bpl = api.context_info()
    contigs, specs = CC.seam_case(bpw, bpl)
    assert len(specs) == 6 and {s.kind for s in specs} == {A.CTX_PERIOD, A.CTX_GC}
    off = np.cumsum([0] + [len(c) for c in contigs])
    assert off[1] % bpw == 0 and off[2] % bpw == 0 and off[3] % bpl != 0
    rows = CM.all_intervals(contigs, specs)
    want = CC.seam_positions(bpw, bpl)
    assert len(want) == 3 * (CC.SEAM_BELOW // bpl - 1) and bpw + 1 in want and bpl - 1 in want
    assert CC.intervals_cover(rows[0][:2] + rows[0][2:], want, "start") == set(want)
    assert CC.intervals_cover(rows[1][:2] + rows[1][2:], want, "stop") == set(want)
    # (the first two contigs alone, whose coordinates are the kernels', carry two of the three offsets each way)
    assert len(CC.intervals_cover(rows[0][:2], want, "start")) >= 2 * len(want) // 3
    longest = lambda k: max(int((r[1] - r[0]).max()) for r in rows[k] if len(r[0]))
    assert longest(0) >= 40000 > 2 * 4 * bpw and longest(4) > bpw
    assert any(int((r[1] - r[0]).max()) > 2 * bpw for r in [rows[0][0]])
    assert all(len(rows[k][c][0]) > 0 for k in range(6) for c in range(3))


@pytest.fixture(scope="module")
def words(tmp_path_factory):
    return CC.words_case(tmp_path_factory.mktemp("context_words"))


def test_words_case_is_not_vacuous(words):
    w = words
    loc, v = w["loc"], w["v"]
    assert len(w["beds"]) == 81 and sum(v.n_vars(h) for h in range(4)) > 3000
    for k in range(70, 81):
        assert any((loc[h][k] == M.INSIDE).any() for h in range(4)), w["names"][k - 70]
        assert len(w["rows"][k - 70][0][0]) > 0
    assert any((loc[h][70:] == M.BORDER).any() for h in range(4))
    assert any((loc[h][70:] == M.OUTSIDE).any() for h in range(4))
