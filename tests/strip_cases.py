"""Alignments aimed at the places where the dense level's column strips (pr_strip.hip: k_strip_plan, k_fwd_strip, k_bwd_strip) differ
from the one-workgroup kernels: where a cut may fall, what crosses it, and the 64-row blocks the boundary columns are published in.

This module holds
  * plan_strips(): k_strip_plan restated over a batch's pointer and flag arrays (the swap sources of a cell as k_prep_cand,
    pr_kernels.hip, ranks them); ST_CAP and the host's slot count are read out of the sources, so a changed constant moves the
    cases with it;
  * the case builders and the table.  Every case is one supercluster over a random contig; its region is the smallest that still
    shows its edge: one or two strips (ST_CAP + ~100 reference bases), three only where a middle strip is the point.  A case
    carries its expectation -- the planner's `ok` code and the number of strips of its first query haplotype -- and what it aims at.
    To keep the oracle cheap the second truth haplotype of a tall case carries one SV-sized deletion of nearly the whole region,
    so two of the four alignments have a handful of rows (the row-block family is made of such haplotypes on purpose).
It imports no product code beyond _abi; tests/test_strip_cases.py shows on the CPU that the table is what it claims,
tests/test_gpu_strips.py runs it through the kernels.

The five conditions.  test_strip_cases.py asks of every condition of the planner that the model without it cuts some case of the
table elsewhere.  The two plane capacities and the pointer equalities are separated by cases of the table.  The two single-source
tests (the cell behind the cut, in either plane, has no swap source but the cell in front of it) are not: on every pointer array
generate_ptrs_strs writes they follow from the pointer equalities -- a second source of REF cell r is a QUERY position x < q - 1
with q2r[x] == r - 1 == q2r[q - 1], so q - 1 is an inserted base and r2q[r - 1] points in front of the insertion, not to q - 1 -- and
400 random clusters of SNPs, insertions and deletions packed around the natural cut found no counterexample.  They guard Level A
arrays a caller made by other means; EDITED holds two such arrays (the plain case's, with one pointer repeated), which only the
model ever sees.

The slot limit.  k_strip_plan also refuses when an alignment needs more strips than the host gave it slots
(2 * ceil(max(Lq, Lr) / ST_CAP) + 2).  The scan takes the furthest admissible column, so two neighbouring strips never fit one
strip together: their REF columns or their QUERY columns exceed ST_CAP.  That allows strips of half of ST_CAP in ONE plane each:
overflow_query(n) is n deletions of ST_CAP / 2 + 1 bases and then n insertions of as many, 2 n - 1 strips over planes of
(n / 2) * ST_CAP columns.  search_slot_overflow() tries n = 1 .. 8 and finds the first input whose cuts outnumber the slots at
n = 5 (nine strips, eight slots; planes of 10 585 columns): the case slots_overflow, with two short truth haplotypes so that the
oracle takes a second."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

import oracle_lib as O
from vcfdist_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vcfdist_amd", "csrc")
_BASES = np.frombuffer(b"ACGT", np.uint8)
PAD = 30                # contig bases outside the region, on either side


# ----------------------------------------------------------------------------------------------------------------------
# constants, read out of the sources
# ----------------------------------------------------------------------------------------------------------------------
def _constants():
    """-> (ST_CAP, slots(Lq, Lr), the formula's text) from pr_strip.hip and strip_plan (pr_api.hip)"""
    strip = open(os.path.join(CSRC, "pr_strip.hip")).read()
    api = open(os.path.join(CSRC, "pr_api.hip")).read()
    nt = int(re.search(r"#define ST_NT (\d+)", strip).group(1))
    c = int(re.search(r"#define ST_C (\d+)", strip).group(1))
    m = re.search(r"#define ST_CAP \(ST_NT \* ST_C - (\d+)\)", strip)
    cap = nt * c - int(m.group(1))
    f = re.search(r"slots_of = \[\]\(const AlnDesc &d\) \{ return (\d+) \* \(\(std::max\(d\.Lq, d\.Lr\) \+ ST_CAP - 1\) / ST_CAP\) \+ (\d+); \}", api)
    a, b = int(f.group(1)), int(f.group(2))
    return cap, (lambda Lq, Lr: a * ((max(Lq, Lr) + cap - 1) // cap) + b), f.group(0)


ST_CAP, slots_of, SLOTS_TEXT = _constants()
STRIP_MIN = 2049        # CLASSES[STRIP_CLS - 1].max_cols + 1 (pr_host.h): narrower alignments never reach the planner
CONDITIONS = ("cap_q", "cap_r", "ptr_eq", "single_r", "single_q")


# ----------------------------------------------------------------------------------------------------------------------
# the planner, restated
# ----------------------------------------------------------------------------------------------------------------------
def fwd_allow(flag):
    """fwd_allow (pr_kernels.hip): a swap may leave a position outside a variant, or on a variant's last position"""
    flag = np.asarray(flag)
    return ((flag & A.PTR_VARIANT) == 0) | ((flag & A.PTR_VAR_END) != 0)


def swap_sources(ptr, flag, n_dst):
    """k_prep_cand -> (first, second): per destination d of the other plane its first two swap sources -- the positions x with
    ptr[x] + 1 == d and fwd_allow(flag[x]), in ascending order -- or -1"""
    ptr = np.asarray(ptr, np.int64)
    first, second = np.full(n_dst, -1, np.int64), np.full(n_dst, -1, np.int64)
    d = ptr + 1
    for x in np.flatnonzero(fwd_allow(flag) & (d >= 1) & (d < n_dst)):
        if first[d[x]] < 0:
            first[d[x]] = x
        elif second[d[x]] < 0:
            second[d[x]] = x
    return first, second


def hap_arrays(batch, sc, qs):
    """-> (q2r, qflag, r2q, rflag) of query haplotype qs of supercluster sc"""
    qo, ro = batch.hap_off[qs], batch.ref_off
    return (batch.hap_ptr[qs][qo[sc]:qo[sc + 1]], batch.hap_flag[qs][qo[sc]:qo[sc + 1]],
            batch.ref_ptr[qs][ro[sc]:ro[sc + 1]], batch.ref_flag[qs][ro[sc]:ro[sc + 1]])


def plan_strips(batch, sc, aln, drop=None, slots=None):
    """k_strip_plan for alignment aln = 2 * query hap + truth hap of supercluster sc -> [(lo_q, lo_r, hi_q, hi_r)] or None (no
    cut, or more strips than slots).  drop: one of CONDITIONS, left out (the discrimination check of test_strip_cases.py)."""
    q2r, qflag, r2q, rflag = hap_arrays(batch, sc, aln >> 1)
    Lq, Lr = len(q2r), len(r2q)
    max_n = slots_of(Lq, Lr) if slots is None else slots
    cr, cr2 = swap_sources(q2r, qflag, Lr)          # cand_r: sources in the QUERY plane, destinations in the REF plane
    cq, cq2 = swap_sources(r2q, rflag, Lq)
    r_lo = q_lo = 0
    out = []
    while True:
        if len(out) >= max_n:
            return None
        if Lr - r_lo <= ST_CAP and Lq - q_lo <= ST_CAP:
            out.append((q_lo, r_lo, Lq, Lr))
            return out
        fr = fq = -1
        for r in range(min(r_lo + ST_CAP, Lr - 1), r_lo, -1):
            q = int(r2q[r])
            if q <= q_lo:
                break
            if (q - q_lo > ST_CAP and drop != "cap_q") or q >= Lq:
                continue
            if drop != "ptr_eq" and (r2q[r - 1] != q - 1 or q2r[q] != r or q2r[q - 1] != r - 1):
                continue
            if drop != "single_r" and not (cr[r] < 0 or (cr[r] == q - 1 and cr2[r] < 0)):
                continue
            if drop != "single_q" and not (cq[q] < 0 or (cq[q] == r - 1 and cq2[q] < 0)):
                continue
            fr, fq = r, q
            break
        if fr < 0:
            return None
        out.append((q_lo, r_lo, fq, fr))
        r_lo, q_lo = fr, fq


def plan_strips_no_cap_r(batch, sc, aln):
    """plan_strips with the REF plane's capacity test removed: the scan starts at the plane's last column"""
    q2r, qflag, r2q, rflag = hap_arrays(batch, sc, aln >> 1)
    Lq, Lr = len(q2r), len(r2q)
    cr, cr2 = swap_sources(q2r, qflag, Lr)
    cq, cq2 = swap_sources(r2q, rflag, Lq)
    r_lo = q_lo = 0
    out = []
    while len(out) < slots_of(Lq, Lr):
        if Lr - r_lo <= ST_CAP and Lq - q_lo <= ST_CAP:
            return out + [(q_lo, r_lo, Lq, Lr)]
        for r in range(Lr - 1, r_lo, -1):
            q = int(r2q[r])
            if q <= q_lo:
                return None
            if q - q_lo > ST_CAP or q >= Lq or r2q[r - 1] != q - 1 or q2r[q] != r or q2r[q - 1] != r - 1:
                continue
            if not (cr[r] < 0 or (cr[r] == q - 1 and cr2[r] < 0)) or not (cq[q] < 0 or (cq[q] == r - 1 and cq2[q] < 0)):
                continue
            break
        else:
            return None
        out.append((q_lo, r_lo, q, r))
        r_lo, q_lo = r, q
    return None


def model_without(cond):
    """the model with one of CONDITIONS removed -> f(batch, sc, aln)"""
    if cond == "cap_r":
        return plan_strips_no_cap_r
    return lambda batch, sc, aln: plan_strips(batch, sc, aln, drop=cond)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
# A variant is ("S", pos[, k]) | ("I", pos, n | -n | bases) | ("D", pos, n); pos counts from the region's first base.  A SNP's alternate
# base is the reference base rotated by k (1..3) in ACGT, drawn when k is left out (the same k on two haplotypes: a shared SNP).
# q / q2: the query haplotypes (q2 None: homozygous); t / t2: the truth's (t2 None: one deletion of all but TINY_ROWS bases)
# edit: [(pos, bytes)] written into the contig before the variants are read off it (N, lower case)
# embed: (window_edge_cases case, offset): that module's tandem-tract construction -- contig piece and variants of all four
#   haplotypes -- laid into the region from `offset` on (family ties)
# ok / n_strips: what the planner must decide for the alignments of the FIRST query haplotype, ok2 / n2: of the second;
# aim: what the case is there for
Case = namedtuple("Case", "name family L q q2 t t2 edit embed ok n_strips ok2 n2 aim")
TINY_ROWS = 40


def _case(name, family, L, q=(), t=(), q2=None, t2=None, edit=(), embed=None, ok=1, n_strips=2, ok2=None, n2=None, aim=""):
    return Case(name, family, L, tuple(q), None if q2 is None else tuple(q2), tuple(t), None if t2 is None else tuple(t2), tuple(edit),
                embed, ok, n_strips, ok if ok2 is None else ok2, n_strips if n2 is None else n2, aim)


def _variants(rng, contig, beg, specs):
    out = []
    for s in sorted(specs, key=lambda s: s[1]):
        p = beg + s[1]
        if s[0] == "S":
            k = s[2] if len(s) > 2 else int(rng.randint(1, 4))
            up = contig[p] & 0xdf
            alt = "ACGT"[(b"ACGT".index(up) + k) % 4] if up in b"ACGT" else "ACGT"[k]
            out.append((p, A.TYPE_SUB, chr(contig[p]), alt, 30.0))
        elif s[0] == "I":
            if isinstance(s[2], str):
                alt = s[2]
            elif s[2] > 0:
                alt = bytes(rng.choice(_BASES, s[2])).decode()
            else:       # -n: n times a base that is neither neighbour's, so that no other placement of the insertion costs the same
                alt = chr([c for c in b"ACGT" if c not in (contig[p - 1] & 0xdf, contig[p] & 0xdf)][0]) * -s[2]
            out.append((p, A.TYPE_INS, "", alt, 30.0))
        else:
            out.append((p, A.TYPE_DEL, bytes(contig[p:p + s[2]]).decode(), "", 30.0))
    return out


def build(case, ctg=0):
    """-> (contig, supercluster dict) of one case, reproducible from its name; the region holds case.L reference bases"""
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    contig = bytearray(rng.choice(_BASES, case.L + 2 * PAD).tobytes())
    for pos, b in case.edit:
        contig[PAD + pos:PAD + pos + len(b)] = b
    extra = [[], [], [], []]
    if case.embed is not None:
        import window_edge_cases as W
        wc, off = case.embed
        piece = W.build(wc)
        body = piece.contig[piece.sc["beg"]:piece.sc["end"]].encode()
        contig[PAD + off:PAD + off + len(body)] = body
        shift = PAD + off - piece.sc["beg"]
        extra = [[(p + shift, ty, r, a, ql) for p, ty, r, a, ql in vs] for vs in piece.sc["vars"]]
    t2 = case.t2 if case.t2 is not None else (("D", TINY_ROWS // 2, case.L - TINY_ROWS),)
    vs = [sorted(_variants(rng, contig, PAD, v) + x)
          for v, x in zip((case.q, case.q if case.q2 is None else case.q2, case.t, t2), extra)]
    return contig.decode(), dict(ctg=ctg, beg=PAD, end=PAD + case.L - 1, vars=vs)      # (end: inclusive)


def batch_of(cases):
    """one batch, a contig and a supercluster per case -> (Variants, Batch)"""
    built = [build(c, ctg=i) for i, c in enumerate(cases)]
    v = A.Variants.from_sites([b[0] for b in built], [b[1] for b in built])
    return v, O.generate(v)


def overflow_query(n):
    """A query haplotype whose cuts outnumber the host's slots: n deletions of ST_CAP / 2 + 1 bases, then n insertions of as many,
    30 bases apart.  Two deletions do not fit one strip's REF columns and two insertions not its QUERY columns, so every strip holds
    one of them but the strip with the last deletion and the first insertion: 2 n - 1 strips over planes of about (n / 2) * ST_CAP
    columns, against 2 * ceil(n / 2 + ...) + 2 slots.  -> (L, variants)"""
    h = ST_CAP // 2 + 1
    q, pos = [], 30
    for _ in range(n):
        q.append(("D", pos, h))
        pos += h + 30
    for _ in range(n):
        q.append(("I", pos, h))
        pos += 30
    return pos + 30, q


def search_slot_overflow(n_max=8):
    """the smallest n whose overflow_query needs more strips than the host's slot count -> (n, strips needed, slots), or None"""
    for n in range(1, n_max + 1):
        L, q = overflow_query(n)
        _, b = batch_of([_case(f"overflow_search_{n}", "slots", L, q=q, t2=())])
        Lq, _, _, _, Lr = b.lens(0)
        need = plan_strips(b, 0, 0, slots=1 << 20)
        if need is not None and len(need) > slots_of(Lq, Lr):
            return n, len(need), slots_of(Lq, Lr)
    return None


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
C_ = ST_CAP
L2 = ST_CAP + 112           # two strips: the second one 112 columns wide
L3 = 2 * ST_CAP + 112       # three strips
OVERFLOW_N = 5              # (search_slot_overflow()'s answer; test_strip_cases.py checks it)


def _rows(L, n):
    """a truth haplotype of n bases over a region of L: one deletion of the rest, behind the first n // 2 bases"""
    return (("D", max(n // 2, 1), L - n),)


def _table():
    import window_edge_cases as W
    out = []
    c = lambda *a, **k: out.append(_case(*a, **k))
    # ---- 1. widths (the planes are as long as the region: no query variant)
    c("width_2049", "widths", STRIP_MIN, n_strips=1, aim="the narrowest alignment the planner sees: one strip, no neighbour")
    c("width_cap", "widths", C_, n_strips=1, aim="the widest single strip: every thread but the last two holds real cells")
    c("width_cap+1", "widths", C_ + 1, n_strips=2, aim="a last strip of one column (its ghost and one real cell)")
    c("width_2cap-1", "widths", 2 * C_ - 1, n_strips=2, aim="two strips, the second one column short of full")
    c("width_2cap+1", "widths", 2 * C_ + 1, n_strips=3, aim="a third strip of one column behind two full ones")
    # ---- 2. cut alignment: lo modulo 4, per plane (bal = max(lo - 1, 0) & ~3: which of thread 0's cells is the ghost)
    c("residue_q0_r0", "residue", L2, aim="cut at (ST_CAP, ST_CAP): the ghost is thread 0's last cell in both planes")
    for k in (1, 2, 3):
        c(f"residue_ins{k}_del{k}", "residue", L2, q=[("I", 700, k)], q2=[("D", 700, k)],
          aim=f"hap 1: {k} inserted bases in front: the QUERY plane fills first, lo = (ST_CAP, ST_CAP - {k}); hap 2: {k} deleted: lo = (ST_CAP - {k}, ST_CAP)")
    for k in (1, 2, 3):
        c(f"residue_block{k}", "residue", L2, q=[("D", C_ - k + 1, k)],
          aim=f"a deletion of {k} on the natural cut: lo = ST_CAP - {k} in both planes")
    # ---- 3. the cut pushed back
    c("push_ins_del", "push", L2, q=[("I", C_ - 3, 5), ("D", C_ + 2, 4)], aim="an insertion in front of the natural cut and a deletion behind it")
    ins300 = bytes(np.random.RandomState(300).choice(_BASES, 300)).decode()
    c("push_cap_q", "push", L2, q=[("I", 2000, ins300)], t=[("I", 2000, ins300)],
      aim="300 inserted bases, shared with the truth: the q - q_lo > ST_CAP branch skips 300 REF columns")
    c("push_snp_on", "push", L2, q=[("S", C_)], t=[("S", C_ - 40)], aim="a query SNP on the cut column (first column of strip 1)")
    c("push_snp_before", "push", L2, q=[("S", C_ - 1)], t=[("S", C_ - 40)], aim="a query SNP on the ghost column")
    c("push_snp_behind", "push", L2, q=[("S", C_ + 1)], t=[("S", C_ - 40)], aim="a query SNP one behind the cut column")
    c("push_no_source", "push", L2, q=[("I", C_ - 2, 2)], aim="an insertion ending on the ghost: the cells behind it have no swap source; the cut moves in front of it")
    c("push_adjacent_dels", "push", L2, q=[("D", C_ - 4, 2), ("D", C_ - 2, 2)], q2=[("D", C_ - 2, 2), ("S", C_)],
      aim="adjacent deletion records next to the cut: the cell behind them has three swap sources")
    c("push_ins_next_to_del", "push", L2, q=[("I", C_ - 3, 2), ("D", C_ - 2, 2)],
      aim="an insertion one base in front of a deletion: three columns behind them every cell has one swap source, the cell in front "
          "of it, and only the pointer equalities refuse the cut")
    # ---- 4. no cut at all
    c("nocut_ins", "nocut", 120, q=[("I", 50, C_ + 1)], t=[("S", 60)], t2=[("S", 80)], ok=0, n_strips=0,
      aim="a query insertion longer than a strip: left to the one-workgroup kernels")
    c("nocut_del", "nocut", C_ + 150, q=[("D", 50, C_ + 1)], t=[("S", 60)], ok=0, n_strips=0, aim="a query deletion longer than a strip")
    # ---- 5. row blocks: the boundary columns are published in blocks of 64 rows
    for a, b in ((2, 63), (64, 65), (127, 128), (129, 1)):
        c(f"rows_{a}_{b}", "rows", L2, t=_rows(L2, a), t2=_rows(L2, b), aim=f"truth haplotypes of {a} and {b} rows: thousands of in-row INS steps across the cut")
    c("rows3_64_65", "rows", L3, t=_rows(L3, 64), t2=_rows(L3, 65), n_strips=3, aim="one block, and one block and a row, through a middle strip")
    # ---- 6. what crosses the cut on the optimal path
    c("cross_mat", "cross", L2, aim="MAT")
    c("cross_sub", "cross", L2, t=[("S", C_)], aim="SUB")
    c("cross_del", "cross", L2, t=[("I", C_, -3)], aim="DEL")                 # (three truth bases consumed on the ghost column)
    c("cross_del_behind", "cross", L2, t=[("I", C_ + 1, -3)], aim="DEL")      # (on the cut column)
    c("cross_ins", "cross", L2, t=[("D", C_ - 2, 5)], aim="INS")
    c("cross_swap_q2r", "cross", L2, q=[("S", C_ - 1, 1), ("S", C_, 1)], t=[("S", C_ - 1, 1)], aim="SWAP_Q2R")
    c("cross_swap_r2q", "cross", L2, q=[("S", C_ - 1, 1), ("S", C_, 1)], t=[("S", C_, 1)], aim="SWAP_R2Q")
    # ---- 7. container-order ties (2k == u, window_edge_cases.py) in a strip with a left neighbour
    tie = W._case("priced", 16, 4, 1, k=2)
    c("tie_behind_cut", "ties", L2 + 100, embed=(tie, C_ + 4 - W.FLANK), t2=(), aim="the tied swap sources a few columns behind the cut")
    c("tie_middle_strip", "ties", L3, embed=(tie, C_ + 1500), t2=(), n_strips=3, aim="the same in a middle strip")
    # ---- 8. block skipping under the window level's upper bound
    # (the oracle's time goes with rows x distance: a deletion shared by query and truth takes most of the rows away at no cost)
    c("ub_strip0", "ub", L2, q=[("D", 600, 3300)], t=[("D", 20, 560), ("D", 600, 3300)],
      aim="a truth-only deletion of 560 bases, more than the 1 024-cell window holds, in strip 0")
    c("ub_strip1", "ub", C_ + 800, q=[("D", 200, 3800)], t=[("D", 200, 3800), ("D", C_ + 100, 560)],
      aim="the same in strip 1: the two strips skip different blocks")
    # ---- 9. other bytes
    c("bytes_n_lower", "bytes", L2, edit=[(C_ - 3, b"acg"), (C_, b"N"), (C_ + 1, b"tt")], t=[("S", C_ - 2)], aim="N on the cut column, lower case around it")
    # ---- more cuts than slots
    Lo, qo = overflow_query(OVERFLOW_N)
    c("slots_overflow", "slots", Lo, q=qo, t=_rows(Lo, 130), t2=_rows(Lo, 70), ok=0, n_strips=0,
      aim="nine strips needed, eight slots given: the planner refuses, the one-workgroup kernels take it")
    return out


TABLE = _table()
FAMILIES = ("widths", "residue", "push", "nocut", "rows", "cross", "ties", "ub", "bytes", "slots")


def edited(which):
    """-> a batch for the MODEL only (see the module's text): the plain two-strip case with one pointer in front of the natural cut
    (ST_CAP, ST_CAP) repeated, so that the cell behind the cut has two swap sources while the four pointer equalities still hold.
    which: "single_r" (a QUERY position) | "single_q" (a REF position)"""
    _, b = batch_of([_case("edited_" + which, "edited", L2)])
    arr = (b.hap_ptr if which == "single_r" else b.ref_ptr)[0]
    assert arr[ST_CAP - 2] == ST_CAP - 2
    arr = arr.copy()
    arr[ST_CAP - 2] = ST_CAP - 1
    (b.hap_ptr if which == "single_r" else b.ref_ptr)[0] = arr
    return b


EDITED = ("single_r", "single_q")


# ----------------------------------------------------------------------------------------------------------------------
# the oracle's results, case by case
# ----------------------------------------------------------------------------------------------------------------------
_FIELDS = ("aln_dist", "aln_end_plane", "aln_beg_plane", "aln_status", "sc_phase", "orig_phase_dist", "swap_phase_dist")
_WANT = {}


def _oracle_of(case):
    _, b = batch_of([case])
    r = O.run(b)
    d = {f: np.array(getattr(r, f)) for f in _FIELDS}
    for name, _ in A.Results.PER_VAR:
        d[name] = [[np.array(getattr(r, name)[h][w]) for w in range(2)] for h in range(4)]
    return case.name, d


def oracle_results(cases):
    """{case name: the oracle's result arrays of the case alone}, computed once per process, on up to eight cores"""
    todo = [c for c in cases if c.name not in _WANT]
    if todo:
        import multiprocessing
        import sys
        n = max(1, min(8, len(os.sched_getaffinity(0)), len(todo)))
        if not os.path.exists(getattr(sys.modules.get("__main__"), "__file__", None) or ""):
            n = 1           # (a spawned worker re-imports __main__: not from a script read from standard input)
        if n > 1:
            O.lib()         # (built once, in the parent)
            # (fresh interpreters, not forks: the GPU tests call this from a process that has the device open)
            with multiprocessing.get_context("spawn").Pool(n) as pool:
                _WANT.update(pool.map(_oracle_of, todo, chunksize=1))
        else:
            _WANT.update(map(_oracle_of, todo))
    return {c.name: _WANT[c.name] for c in cases}


def expected(cases, batch):
    """the oracle's Results of the batch of `cases`, put together from the cases' own runs (superclusters are independent: every
    array is per supercluster or per variant of one)"""
    per = oracle_results(cases)
    r = A.Results.for_batch(batch)
    for f in _FIELDS:
        getattr(r, f)[:] = np.concatenate([per[c.name][f] for c in cases])
    for name, _ in A.Results.PER_VAR:
        for h in range(4):
            for w in range(2):
                getattr(r, name)[h][w][:] = np.concatenate([per[c.name][name][h][w] for c in cases])
    return r


# ----------------------------------------------------------------------------------------------------------------------
# what the oracle's path does at a cut
# ----------------------------------------------------------------------------------------------------------------------
def crossing_edges(batch, sc, aln, plan):
    """-> (edges, dels): per cut of `plan` the edge of the oracle's path that leads from a strip into its right neighbour -- MAT,
    SUB, INS, SWAP_Q2R or SWAP_R2Q -- and the number of DEL steps (a truth base consumed, same column) the path takes on the
    cut column or on the column in front of it"""
    ex = O.Extra(batch, want=(sc, aln))
    O.run(batch, extra=ex)
    pl, x, t, _, _ = ex.path_arrays()
    order = np.lexsort((x, t)) if len(t) > 1 and t[0] > t[-1] else np.arange(len(t))
    pl, x, t = pl[order].astype(int), x[order].astype(int), t[order].astype(int)
    qs, ts = aln >> 1, 2 + (aln & 1)
    seqs = (batch.hap_seq[qs][batch.hap_off[qs][sc]:batch.hap_off[qs][sc + 1]], batch.ref_seq[batch.ref_off[sc]:batch.ref_off[sc + 1]])
    truth = batch.hap_seq[ts][batch.hap_off[ts][sc]:batch.hap_off[ts][sc + 1]]
    edges, dels = [], []
    for lo_q, lo_r, _, _ in plan[1:]:
        lo = (lo_q, lo_r)
        kind, n_del = None, 0
        for k in range(len(t) - 1):
            a, b = (pl[k], x[k], t[k]), (pl[k + 1], x[k + 1], t[k + 1])
            if a[0] == b[0] and a[1] == b[1] and a[1] in (lo[a[0]] - 1, lo[a[0]]):
                n_del += 1
            if a[1] < lo[a[0]] and b[1] >= lo[b[0]]:
                assert kind is None and a[1] == lo[a[0]] - 1 and b[1] == lo[b[0]], (a, b, lo)
                if a[0] != b[0]:
                    kind = "SWAP_Q2R" if a[0] == A.PLANE_QUERY else "SWAP_R2Q"
                elif a[2] == b[2]:
                    kind = "INS"
                else:
                    kind = "MAT" if seqs[b[0]][b[1]] == truth[b[2]] else "SUB"
        edges.append(kind)
        dels.append(n_del)
    return edges, dels
