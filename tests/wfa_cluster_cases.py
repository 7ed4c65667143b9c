"""Clusterings aimed at the places where the biWFA dependency clustering (vcfdist_amd/csrc/wfa_cluster.hip: k_wfa_align, k_wfa_reach
and the host rounds around them) can be wrong without a random contig noticing: the five size classes a job is sorted into, the
64-lane stride over the diagonals, the ring of wavefront rows, the doubling rounds and the contig's ends, the main diagonal's stop,
and the host's merge passes.

This module holds
  * the first-round job arithmetic of vcl_wfa_cluster restated in plain Python from the text of wfa_cluster.hip -- the window of
    a side in doubling round k, q_len, r_len, mat_len, need_bytes and the size class (jobs_of) -- a plain affine-gap DP for a
    cluster's score (gap_score), and wf_swg_max_reach restated with the diagonal of its first hit (reach_trace).  None of it calls
    project code;
  * the case builders and the table.  A case is one small contig (seeded random sequence, tandem tracts planted where a reach has
    to run), the variants of one haplotype, a penalty set, the iteration limits it is run with, what it is aimed at, and what it
    declares: tests/test_wfa_cluster_cases.py shows on the CPU that every case is what it declares, tests/test_gpu_wfa_cluster_edges.py
    runs the table through the kernels, tests/golden/make_ref_goldens.py (set cluster_edges) records the reference's answers.
Every case stays clear of undefined input: no overlapping records, no cluster with an empty query, and no variant at position 0 or
on the last base outside the edge_* cases written for that.

Scores the penalties cannot make.  A cluster's score is a sum of x (a SNP) and o + n e (an indel of n); `scores` = max(x, o + e) + 1
itself is out of reach at 5/6/2 (5, 8, 10, 12, 13, ...), 4/3/2 (4, 5, 7, 8, ...) and 8/6/2, so ring_* takes, per penalty set, the
largest score below the ring length, the ring length where a cluster can have it, and the smallest score above it, and says which.

The stale SUB value.  k_wfa_reach starts a reused slot's SUB entry at its old value because the reference does.  No case of this
table shows it, and none was found that does.  The reason, as far as it is understood (an argument, not a proof): an entry on a
diagonal has a successor on the same diagonal x <= rows - 1 scores later with an offset at least as large (were it at the query's or
the truth's end it would have been a hit, which returns), so the old value should never win a comparison or the final maximum.
tests/golden/README.md has the scratch run of the kernel without it (nothing fails) and says exactly what was changed in the oracle
for the random comparison (no difference).  A case that tells the two apart, if one exists, is still missing."""
import zlib
from collections import namedtuple

import numpy as np

S, I, D = 1, 2, 3
LIM = (8 << 10, 16 << 10, 32 << 10, 64 << 10)          # dynamic LDS of the four LDS launches (wfa_cluster.hip: LIM)
N_CLASSES = 5
GLOBAL = 4
PENALTIES = ((5, 6, 2), (3, 2, 1), (4, 3, 2), (1, 1, 1), (9, 2, 1), (1, 3, 2))          # make_ref_goldens.PENALTIES
PEN_EQ = (8, 6, 2)                                                                      # x == o + e
PEN_OPEN0 = (3, 0, 1)                                                                   # -o 0: the reference's parser takes it
PEN_EXACT = (5, 4, 2)          # a ring of 7 rows: the only ring length (2 .. 13) at which a job can need exactly one of the four limits
DEFAULT = (5, 6, 2)
_BASES = "ACGT"


# ----------------------------------------------------------------------------------------------------------------------
# the job arithmetic, restated
# ----------------------------------------------------------------------------------------------------------------------
Job = namedtuple("Job", "kind round q_len r_len mat_len need_bytes cls q_beg q_end r_beg")


def ring_rows(pen):
    x, o, e = pen
    return max(x, o + e) + 1


def need_bytes(q_len, r_len, pen):
    return 4 * (((q_len + 3) >> 2) + ((r_len + 3) >> 2) + 3 * ring_rows(pen) * (q_len + r_len - 1))


def size_class(nb):
    for b, lim in enumerate(LIM):
        if nb <= lim:
            return b
    return GLOBAL


def gen_len(variants, beg, end, ctg_len):
    """length of generate_str over [beg, end) with the cluster's variants applied (all of them lie inside)"""
    n = min(end, ctg_len) - beg
    for p, t, ref, alt in variants:
        assert beg <= p and p + len(ref) <= end
        n += len(alt) - len(ref)
    return n


def _job(kind, rnd, variants, q_beg, q_end, r_beg, r_len, ctg_len, pen):
    q = gen_len(variants, q_beg, q_end, ctg_len)
    nb = need_bytes(q, r_len, pen)
    return Job(kind, rnd, q, r_len, q + r_len - 1, nb, size_class(nb), q_beg, q_end, r_beg)


def cluster_span(variants):
    """beg_pos, end_pos, main_diag of a cluster: one base in front of its first variant, one behind its last"""
    p0 = variants[0][0]
    pl, _, rl, _ = variants[-1]
    return p0 - 1, pl + len(rl) + 1, sum(len(r) - len(a) for _, _, r, a in variants)


def align_job(variants, ctg_len, pen):
    beg, end, _ = cluster_span(variants)
    q_beg, q_end = max(0, beg), min(ctg_len, end)
    return _job("align", 0, variants, q_beg, q_end, q_beg, q_end - q_beg, ctg_len, pen)


def reach_job(variants, ctg_len, pen, score, reverse, rnd):
    """the job of one side in doubling round rnd = 1, 2, ...: the window has 2^rnd times the cluster's span"""
    beg, end, md = cluster_span(variants)
    e = pen[2]
    ref_len = (end - beg) << rnd
    slack = abs(md) + score // e + 3
    if reverse:
        q_beg = max(0, end - ref_len - slack)
        r_beg = max(0, end - ref_len)
        return _job("rev", rnd, variants, q_beg, end, r_beg, min(ref_len, ctg_len - r_beg), ctg_len, pen)
    q_end = min(ctg_len, beg + ref_len + slack)
    return _job("fwd", rnd, variants, beg, q_end, beg, min(ref_len, q_end - beg, ctg_len - beg), ctg_len, pen)


def jobs_of(variants, ctg_len, pen, score, rounds=(1, 1)):
    """every job of an active cluster in one iteration: its align job, `rounds[0]` reverse and `rounds[1]` forward reach jobs"""
    out = [align_job(variants, ctg_len, pen)]
    out += [reach_job(variants, ctg_len, pen, score, True, k) for k in range(1, rounds[0] + 1)]
    out += [reach_job(variants, ctg_len, pen, score, False, k) for k in range(1, rounds[1] + 1)]
    return out


def apply_variants(ctg, variants, beg, end):
    out, p = [], beg
    for pos, t, ref, alt in variants:
        assert pos >= p, "records overlap"
        out.append(ctg[p:pos]); out.append(alt); p = pos + len(ref)
    out.append(ctg[p:end])
    return "".join(out)


def gap_score(q, t, pen):
    """plain affine-gap global alignment cost (match 0, mismatch x, a gap of n: o + n e) -- what wf_swg_align returns"""
    x, o, e = pen
    INF = 1 << 30
    n = len(t)
    M = [0] + [o + j * e for j in range(1, n + 1)]
    Dg = [INF] * (n + 1)                                  # gap in q (consumes t)
    Ig = list(M); Ig[0] = INF
    for i in range(1, len(q) + 1):
        m2, d2, i2 = [INF] * (n + 1), [INF] * (n + 1), [INF] * (n + 1)
        d2[0] = min(Dg[0], M[0] + o) + e
        m2[0] = d2[0]
        qc = q[i - 1]
        for j in range(1, n + 1):
            d2[j] = min(Dg[j], M[j] + o) + e
            i2[j] = min(i2[j - 1], m2[j - 1] + o) + e
            s = M[j - 1] + (0 if qc == t[j - 1] else x)
            m2[j] = min(s, d2[j], i2[j])
        M, Dg, Ig = m2, d2, i2
    return M[n]


def cluster_score(ctg, variants, pen):
    beg, end, _ = cluster_span(variants)
    beg, end = max(0, beg), min(len(ctg), end)
    return gap_score(apply_variants(ctg, variants, beg, end), ctg[beg:end], pen)


# reach: the answer; d: the diagonal of the first hit (None: no hit, the answer is the ring's maximum); s: the score it ended at;
# hits: (d, value) of every diagonal of that row that hits (the reference returns at the first; a kernel sees a chunk of 64 at once)
Reach = namedtuple("Reach", "reach d s hits")


def reach_trace(query, truth, main_diag, main_diag_start, max_score, pen, reverse):
    """wf_swg_max_reach restated (numpy over the diagonals of a row; nothing in a row depends on another diagonal of the same row)
    -> Reach.  The ring keeps the SUB row of a reused slot and resets
    INS / DEL only; without a hit the answer is the maximum over every slot."""
    x, o, e = pen
    q = np.frombuffer(query.encode(), np.uint8)
    t = np.frombuffer(truth.encode(), np.uint8)
    ql, tl = len(q), len(t)
    y = ql + tl - 1
    rows = ring_rows(pen)
    offs = np.full((3, rows, y), -2, np.int64)
    diag = np.arange(y) + 1 - ql
    mdo = main_diag_start - main_diag
    none = np.array([-2])
    left = lambda a: np.concatenate([none, a[:-1]])          # the value of diagonal d - 1 (none at d == 0)
    right = lambda a: np.concatenate([a[1:], none])          # of diagonal d + 1 (none at d == mat_len - 1)
    inside = lambda off: (off >= 0) & (off < ql) & (diag + off >= 0) & (diag + off < tl)
    s = s2 = 0
    offs[0, 0, ql - 1] = -1
    while True:
        sub = offs[0, s2]
        if not reverse:
            for m in (1, 2):
                off = offs[m, s2]
                k = inside(off) & (off >= sub)
                sub[k] = off[k]
        off = sub.copy()
        go = np.ones(y, bool)
        while True:
            go &= ((diag != main_diag) | (off + 1 < mdo)) & (off != -2) & (diag + off >= -1) & (off < ql - 1) & (diag + off < tl - 1)
            idx = np.flatnonzero(go)
            if not len(idx):
                break
            same = q[off[idx] + 1] == t[diag[idx] + off[idx] + 1]
            off[idx[same]] += 1
            go[idx[~same]] = False
        sub[:] = off
        end_t = off + diag == tl - 1
        end_q = (off == ql - 1) & (off + diag >= 0) & (off + diag < tl - 1)
        hit = np.flatnonzero(end_t | end_q)
        if len(hit):
            d = int(hit[0])
            return Reach(tl - 1 if end_t[d] else int(off[d] + diag[d]), d, s, [(int(k), int(tl - 1 if end_t[k] else off[k] + diag[k])) for k in hit])
        if s == max_score:
            break
        s += 1
        s2 = (s2 + 1) % rows
        offs[1, s2] = -2
        offs[2, s2] = -2
        sub, vins, vdel = offs[0, s2], offs[1, s2], offs[2, s2]          # (sub: the stale row of the reused slot)
        back = e if reverse else o + e
        if s - x >= 0:
            p = offs[0, (s2 - x) % rows]
            k = (p != -2) & (p + 1 < ql) & (diag + p + 1 < tl) & (p + 1 >= sub)
            sub[k] = p[k] + 1
        if s - back >= 0:
            p = left(offs[0, (s2 - back) % rows])
            k = (p != -2) & (diag + p < tl) & (p >= vdel)
            vdel[k] = p[k]
            p = right(offs[0, (s2 - back) % rows])
            k = (p != -2) & (p + 1 < ql) & (diag + p + 1 < tl) & (diag + p + 1 >= 0) & (p + 1 >= vins)
            vins[k] = p[k] + 1
        if reverse and s - o >= 0:
            for m in (1, 2):
                p = offs[m, (s2 - o) % rows]
                k = inside(p) & (p > sub)
                sub[k] = p[k]
        if s - e >= 0:
            p = left(offs[2, (s2 - e) % rows])
            k = (p != -2) & (diag + p < tl) & (p >= vdel)
            vdel[k] = p[k]
            p = right(offs[1, (s2 - e) % rows])
            k = (p != -2) & (p + 1 < ql) & (diag + p + 1 < tl) & (diag + p + 1 >= 0) & (p + 1 >= vins)
            vins[k] = p[k] + 1
    reach = diag[None, None, :] + offs
    ok = (offs >= 0) & (offs < ql) & (reach >= 0) & (reach < tl)
    return Reach(int(reach[ok].max()) if ok.any() else 0, None, s, [])


def side_trace(ctg, variants, pen, score, reverse, rnd=1):
    """reach_trace on the strings of one side's job in round rnd"""
    j = reach_job(variants, len(ctg), pen, score, reverse, rnd)
    beg, end, md = cluster_span(variants)
    q = apply_variants(ctg, variants, j.q_beg, min(j.q_end, len(ctg)))
    t = ctg[j.r_beg:j.r_beg + j.r_len]
    assert len(q) == j.q_len and len(t) == j.r_len
    if reverse:
        q, t = q[::-1], t[::-1]
        mds = end - variants[0][0]
    else:
        mds = variants[-1][0] + len(variants[-1][2]) - beg
    return reach_trace(q, t, md, mds, score, pen, reverse), j


def side_rounds(ctg, variants, pen, score, reverse, limit=12):
    """the doubling rounds of one side, from the restated reach: a reach on the window's last column re-issues the side unless
    the window has met the contig's end -> number of reach calls"""
    for rnd in range(1, limit + 1):
        tr, j = side_trace(ctg, variants, pen, score, reverse, rnd)
        reach = tr.reach
        ref_len = (cluster_span(variants)[1] - cluster_span(variants)[0]) << rnd
        edge = j.q_beg == 0 if reverse else j.q_end == len(ctg)
        if reach != ref_len - 1 or edge:
            return rnd
    raise AssertionError("a side that never settles")


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
# variants: [(pos, type, ref, alt)] of one haplotype, sorted by position
# pen: (x, o, e); itrs: the iteration limits the case is run with
# declare: what the case claims, checked by tests/test_wfa_cluster_cases.py
#   clusters    [[first variant, one past the last]] the final clusters at the largest iteration limit
#   jobs        {(cluster, kind): (mat_len, class)} first-round jobs the case is aimed at (kind: align | rev | fwd)
#   need        {(cluster, kind): need_bytes}
#   score       {cluster: score}; ring: "below" | "at" | "above": the score against the ring length
#   rounds      {cluster: (reverse calls, forward calls)} in the first iteration
#   calls       reach calls of the whole run (doubling_*: the side that slides is re-issued; 2 per cluster where a case says
#               that every side settles in its first window)
#   hit         {(cluster, kind): d} diagonal of the first hit of that first-round reach job; two_values: another diagonal of the
#               same chunk hits with another value; last_diagonal: d is mat_len - 1
#   iterations  {iteration limit: iterations run}
#   undefined   "pos0": input the reference refuses (a fixture of its own); last_base: a variant on the contig's last base
Case = namedtuple("Case", "name group aim ctg variants pen itrs declare")


def _rng(key):
    return np.random.RandomState(zlib.crc32(key.encode()) & 0x7fffffff)


def rand_seq(rng, n):
    """random bases without a run of three equal ones and without a dinucleotide repeated at once: a reach in it stops early"""
    out = []
    while len(out) < n:
        c = _BASES[rng.randint(4)]
        if len(out) >= 2 and out[-1] == c and out[-2] == c:
            continue
        if len(out) >= 3 and out[-1] == out[-3] and out[-2] == c:
            continue
        out.append(c)
    return "".join(out)


def other(c, k=1):
    return _BASES[(_BASES.index(c) + k) % 4]


def snp(ctg, p, k=1):
    return (p, S, ctg[p], other(ctg[p], k))


def dele(ctg, p, n):
    return (p, D, ctg[p:p + n], "")


def ins(ctg, p, n, rng=None, bases=None):
    if bases is None:
        # a base that is neither neighbour's first, so that the insertion cannot slide
        first = [c for c in _BASES if c not in (ctg[p - 1], ctg[p])][0]
        bases = first + rand_seq(rng, n - 1) if n > 1 else first
        if n > 1 and bases[-1] in (ctg[p - 1], ctg[p]):
            bases = bases[:-1] + [c for c in _BASES if c not in (ctg[p - 1], ctg[p], bases[-2])][0]
    return (p, I, "", bases)


def _single(kind, n, pen=DEFAULT):
    """first-round forward reach job of one isolated indel of n bases in unique sequence (nominal score o + n e), far from the
    contig's ends -> Job"""
    ctg_len = 1 << 20
    v = [(1 << 19, D, "A" * n, "")] if kind == "del" else [(1 << 19, I, "", "A" * n)]
    return reach_job(v, ctg_len, pen, pen[1] + n * pen[2], False, 1)


def border_sizes(kind, b, pen=DEFAULT):
    """the largest indel whose first-round reach jobs still fit class b, and the smallest whose do not -> (n_in, n_out)"""
    n = 1
    while _single(kind, n + 1, pen).cls <= b:
        n += 1
    return n, n + 1


def _spread(rng, items, gap=260, lead=300):
    """a contig of random sequence with the clusters of `items` (functions ctg, pos -> variant list; or (function, width)) `gap`
    bases apart -> (ctg, [variant lists])"""
    widths = [it[1] if isinstance(it, tuple) else 8 for it in items]
    total = lead + sum(w + gap for w in widths) + lead
    ctg = rand_seq(rng, total)
    out, p = [], lead
    for it, w in zip(items, widths):
        f = it[0] if isinstance(it, tuple) else it
        out.append(f(ctg, p))
        p += w + gap
    return ctg, out


def _mk(name, group, aim, ctg, clusters, pen=DEFAULT, itrs=(4,), **declare):
    variants = [v for cl in clusters for v in cl]
    assert variants == sorted(variants, key=lambda v: v[0])
    if "clusters" not in declare:
        k, cl_idx = 0, []
        for cl in clusters:
            cl_idx.append([k, k + len(cl)]); k += len(cl)
        declare["clusters"] = cl_idx
    return Case(name, group, aim, ctg, variants, tuple(pen), tuple(itrs), declare)


def case_clusters(case):
    return [case.variants[a:b] for a, b in case.declare["clusters"]]


def predicted_classes(case):
    """jobs per size class of the whole call, for a case of isolated clusters that settle in one iteration: per cluster the
    align job and as many reach jobs a side as the restated reach takes doubling rounds"""
    out = [0] * N_CLASSES
    for cl in case_clusters(case):
        sc = cluster_score(case.ctg, cl, case.pen)
        rounds = tuple(side_rounds(case.ctg, cl, case.pen, sc, rev) for rev in (True, False))
        for j in jobs_of(cl, len(case.ctg), case.pen, sc, rounds):
            out[j.cls] += 1
    return out


# ---- bucket_*
def _bucket_cases():
    out = []
    mixed = []
    for b in range(4):
        for kind in ("del", "ins"):
            n_in, n_out = border_sizes(kind, b)
            for n, side in ((n_in, "in"), (n_out, "out")):
                rng = _rng(f"bucket_{kind}_{b}_{side}")
                f = (lambda ctg, p, n=n: [dele(ctg, p, n)]) if kind == "del" else (lambda ctg, p, n=n, rng=rng: [ins(ctg, p, n, rng)])
                ctg, cls = _spread(rng, [(f, n)], lead=4 * n + 120)
                j = _single(kind, n)
                want = b if side == "in" else b + 1
                assert j.cls == want
                out.append(_mk(f"bucket_{kind}{n}_{LIM[b] >> 10}k_{side}", "bucket",
                               f"one isolated {'deletion' if kind == 'del' else 'insertion'} of {n} bases: its reach jobs have {j.mat_len} diagonals and need "
                               f"{j.need_bytes} bytes, the {'last that fit' if side == 'in' else 'first that do not fit'} the {LIM[b] >> 10} KiB launch",
                               ctg, cls, jobs={(0, "fwd"): (j.mat_len, want), (0, "rev"): (j.mat_len, want)}, need={(0, "fwd"): j.need_bytes},
                               **(dict(calls=2) if kind == "del" else {})))
                if kind == "del" and side == "in" or (b == 3 and kind == "ins" and side == "out"):
                    mixed.append((f, n))
    for kind, n in (("del", 200), ("ins", 300)):
        rng = _rng(f"bucket_global_{kind}")
        f = (lambda ctg, p, n=n: [dele(ctg, p, n)]) if kind == "del" else (lambda ctg, p, n=n, rng=rng: [ins(ctg, p, n, rng)])
        ctg, cls = _spread(rng, [(f, n)], lead=4 * n + 120)
        j = _single(kind, n)
        assert j.cls == GLOBAL and j.need_bytes > 1.5 * LIM[3]
        out.append(_mk(f"bucket_global_{kind}{n}", "bucket", f"well inside the global-scratch class: reach jobs of {j.mat_len} diagonals, {j.need_bytes} bytes",
                       ctg, cls, jobs={(0, "fwd"): (j.mat_len, GLOBAL), (0, "rev"): (j.mat_len, GLOBAL)}))
    # need_bytes == limit.  4 * (ceil(q / 4) + ceil(r / 4) + 3 * rows * (q + r - 1)) equals 8, 16, 32 or 64 KiB for one shape only
    # among rings of 2 .. 13 rows: 7 rows, 771 diagonals, q and r multiples of 4, 64 KiB.  At 5/4/2 the first reach jobs of a
    # 253-base insertion have q = 768, r = 4: the last LDS job by `<=`, a global one by `<`
    rng = _rng("bucket_exact")
    n = 253
    f = lambda ctg, p, rng=rng: [ins(ctg, p, n, rng)]
    ctg, cls = _spread(rng, [(f, n)], lead=4 * n + 120)
    j = _single("ins", n, PEN_EXACT)
    assert j.need_bytes == LIM[3] and (j.q_len, j.r_len, j.mat_len) == (768, 4, 771)
    out.append(_mk("bucket_ins253_exact64k", "bucket", "one isolated insertion of 253 bases at 5/4/2: its first reach jobs need exactly 65 536 bytes, the 64 KiB launch's whole LDS",
                   ctg, cls, pen=PEN_EXACT, jobs={(0, "fwd"): (771, 3), (0, "rev"): (771, 3)}, need={(0, "fwd"): LIM[3], (0, "rev"): LIM[3]}))
    # one contig, all five classes, in an order the stable sort has to undo: global, 8 KiB, 64 KiB, 16 KiB, 32 KiB, and a second
    # global job behind them so that two scratch regions lie apart
    order = [mixed[4], mixed[0], mixed[3], mixed[1], mixed[2], mixed[4]]
    rng = _rng("bucket_mixed")
    ctg, cls = _spread(rng, order, gap=700, lead=900)
    out.append(_mk("bucket_mixed", "bucket", "clusters of all five size classes on one contig, largest first and last: one launch sequence mixes the LDS "
                   "launches with the global variant, the stable sort reorders the jobs, and the global jobs' scratch lies behind LDS jobs' offsets",
                   ctg, cls, itrs=(1, 2, 4)))
    return out


# ---- stride_*
def _find_shape(kind, target, rng, ctg, p):
    """the first cluster whose `kind` job has `target` diagonals: one deletion or insertion of n, else one with a SNP g bases
    behind it (a cluster the second iteration makes) -> (label, variants)"""
    def shapes(n):
        return [(f"del{n}", [dele(ctg, p, n)]), (f"ins{n}", [ins(ctg, p, n, rng)])]
    def pairs(n):
        return [(f"del{n}+snp{g}", [dele(ctg, p, n), snp(ctg, p + n + g)]) for g in (1, 2, 3)] + \
               [(f"ins{n}+snp{g}", [ins(ctg, p, n, rng), snp(ctg, p + g)]) for g in (1, 2, 3)]
    for make in (shapes, pairs):
        for n in range(1, 140):
            for label, v in make(n):
                sc = cluster_score(ctg, v, DEFAULT)
                j = align_job(v, len(ctg), DEFAULT) if kind == "align" else reach_job(v, len(ctg), DEFAULT, sc, kind == "rev", 1)
                if j.mat_len == target:
                    return label, v
    raise AssertionError((kind, target))


def _dup_case(t, k, side="fwd"):
    """a deletion next to the contig's end whose first t bases are the t bases behind it (k of them mutated): the clamped window's
    query ends on truth column t at score k x, on diagonal d == t, before any diagonal reaches the truth's end"""
    name = f"stride_hit_d{t}_s{5 * k}"
    rng = _rng(name)
    T = rand_seq(rng, t)
    Tm = list(T)
    for i in range(k):
        q = (7 + 19 * i) % t
        Tm[q] = other(Tm[q])
    lead = rand_seq(rng, 300)
    if lead[-1] == T[0]:
        lead = lead[:-1] + other(T[0])
    ctg = lead + "".join(Tm) + T
    return _mk(name, "stride", f"a {t}-base deletion whose bases repeat behind it, next to the contig's end: the forward window is cut, the query ends first on "
               f"diagonal {t} (lane {t % 64} of chunk {t // 64}) at score {5 * k}", ctg, [[dele(ctg, 300, t)]], hit={(0, "fwd"): t}, calls=2)


def _stride_cases():
    out = []
    for kind in ("align", "fwd"):
        for target in (63, 64, 65, 127, 128, 129):
            rng = _rng(f"stride_{kind}_{target}")
            ctg = rand_seq(rng, 1400)
            label, v = _find_shape(kind, target, rng, ctg, 700)
            out.append(_mk(f"stride_{kind}_{target}", "stride", f"{label}: the {kind} job has {target} diagonals ({target // 64} chunks of 64 lanes and {target % 64})",
                           ctg, [v], jobs={(0, kind): (target, None)}))
    # first hits.  A hit is the query's end (value: the truth column, which is also the diagonal's index d) or the truth's last
    # column; in a window that is not cut the query is longer than the truth by more than the score pays for, so only a window
    # cut at the contig's end lets the query end first.
    for t in (63, 64):
        for k in (0, 1):
            out.append(_dup_case(t, k))
    # diagonal 0, with a second hit of another value in the same chunk: the lowest lane decides
    rng = _rng("hit0")
    ctg = rand_seq(rng, 60)
    for n, t in ((2, 2), (3, 2), (5, 2)):
        out.append(_mk(f"stride_hit_d0_del{n}", "stride", f"a {n}-base deletion {t} bases in front of the contig's end: the first hit of the cut forward window is on "
                       "diagonal 0 and another diagonal of the same chunk hits with another value", ctg, [[dele(ctg, 60 - n - t, n)]], hit={(0, "fwd"): 0}, two_values=True, calls=2))
    # the last diagonal, d == mat_len - 1: an insertion a few bases in front of the contig's end.  The forward window is cut to
    # r_len = 4 truth bases; diagonal 0 stops on the insertion's first base, and a deletion gap over the other r_len - 1 = 3 truth
    # columns, o + 3 e = 12 <= the cluster's score, is cheaper than three substitutions: the first hit is the truth's last column
    # at offset 0, on the highest diagonal -- in the first, the second and the third chunk of 64 lanes
    rng = _rng("hit_last")
    ctg = rand_seq(rng, 120)
    for n, t in ((3, 4), (60, 3), (130, 4)):
        for k in range(20):         # (inserted bases that match the truth by chance let a shorter gap hit first: the first draw that does not)
            v = [ins(ctg, len(ctg) - t, n, _rng(f"hit_last_{n}_{k}"))]
            tr, j = side_trace(ctg, v, DEFAULT, cluster_score(ctg, v, DEFAULT), False, 1)
            if tr.d == j.mat_len - 1:
                break
        out.append(_mk(f"stride_hit_dlast_ins{n}", "stride", f"a {n}-base insertion {t} bases in front of the contig's end: the cut forward window has {j.mat_len} diagonals and "
                       f"its first hit is on the last one, lane {(j.mat_len - 1) % 64} of chunk {(j.mat_len - 1) // 64}, after a gap over the whole truth",
                       ctg, [v], hit={(0, "fwd"): j.mat_len - 1}, last_diagonal=True))
    return out


# ---- ring_*
def _ring_recipes(pen):
    """cluster recipes by nominal score: k SNPs three bases apart (a SNP costs x, or two one-base gaps where that is cheaper),
    then an indel of n"""
    x, o, e = pen
    out = {}
    for k in range(0, 7):
        for n in range(0, 13):
            for form in ("del", "ins"):
                if k + n == 0 or (n == 0 and form == "ins"):
                    continue
                out.setdefault(k * min(x, 2 * (o + e)) + (o + n * e if n else 0), []).append((k, n, form))
    return out


def _ring_cluster(k, n, form, rng):
    def f(ctg, p):
        v = [snp(ctg, p + 3 * i) for i in range(k)]
        q = p + 3 * k
        if n:
            v.append(dele(ctg, q, n) if form == "del" else ins(ctg, q, n, rng))
        return v
    return (f, 3 * k + n + 2)


def _ring_cases():
    out = []
    for pen in PENALTIES + (PEN_EQ, PEN_OPEN0, PEN_EXACT):
        rows = ring_rows(pen)
        rec = _ring_recipes(pen)
        below = max(s for s in rec if s < rows)
        above = min(s for s in rec if s > rows)
        for tag, target in (("below", below), ("at", rows if rows in rec else None), ("above", above)):
            if target is None:
                continue
            key = f"ring_{pen[0]}{pen[1]}{pen[2]}_{tag}"
            rng = _rng(key)
            picks = sorted(rec[target], key=lambda r: (r[0] + r[1], r))[:5]          # the shortest recipes with that nominal score
            picks = (picks * 16)[:16]
            ctg, cls = _spread(rng, [_ring_cluster(k, n, form, rng) for k, n, form in picks], gap=160, lead=200)
            # (a SNP next to an indel can be cheaper as one longer gap: the plain DP decides, the first ten that score `target` stay)
            cls = [cl for cl in cls if cluster_score(ctg, cl, pen) == target][:10]
            assert len(cls) == 10, key
            out.append(_mk(key, "ring", f"{len(cls)} isolated clusters of score {target} at {pen[0]}/{pen[1]}/{pen[2]}, a ring of {rows} rows: "
                           + {"below": "the last score that reuses no slot", "at": "the first reused slot, row 0 keeps its stale SUB values",
                              "above": "a second reused slot"}[tag] + ("" if tag != "above" or rows in rec else f" (no cluster scores {rows} at these penalties)"),
                           ctg, cls, pen=pen, itrs=(1, 2, 4) if key == "ring_562_above" else (4,), score={c: target for c in range(len(cls))}, ring=tag))
    return out


# ---- doubling_*
def _tract_case(name, aim, unit, reps, at, kind, lead, tail, **kw):
    """an indel of one unit `at` units into a tract unit * reps between random flanks of lead / tail bases"""
    rng = _rng(name)
    a = rand_seq(rng, lead) if lead else ""
    b = rand_seq(rng, tail) if tail else ""
    # the flanks do not continue the tract
    if a and a[-1] == unit[-1]:
        a = a[:-1] + other(a[-1])
    if b and b[0] == unit[0]:
        b = other(b[0]) + b[1:]
    ctg = a + unit * reps + b
    p = lead + at * len(unit)
    v = [dele(ctg, p, len(unit))] if kind == "del" else [(p, I, "", unit)]
    return _mk(name, "doubling", aim, ctg, [v], **kw)


def _doubling_cases():
    out = []
    c = lambda *a, **k: out.append(_tract_case(*a, **k))
    # a deletion of one unit at the tract's start: the forward reach slides along the whole tract, the windows are 2^k * span wide
    c("doubling_dinuc_2", "a 2-base deletion at the start of a 10-base dinucleotide tract", "AC", 5, 0, "del", 400, 400, calls=3)
    c("doubling_dinuc_3", "... of a 24-base tract", "AC", 12, 0, "del", 400, 400, calls=4)
    c("doubling_dinuc_4", "... of a 56-base tract", "AC", 28, 0, "del", 500, 500, calls=5)
    c("doubling_homop_2", "a 1-base deletion at the start of a 7-base homopolymer", "A", 7, 0, "del", 400, 400, calls=3)
    c("doubling_homop_3", "... of a 16-base homopolymer", "A", 16, 0, "del", 400, 400, calls=4)
    c("doubling_homop_4", "... of a 36-base homopolymer", "A", 36, 0, "del", 400, 400, calls=5)
    c("doubling_ins_mid", "a 2-base insertion in the middle of a 60-base dinucleotide tract: both sides are re-issued", "GT", 30, 15, "ins", 500, 500, calls=10)
    # the tract's end against the end of the first forward window (beg_pos + 2 * span: span 4 for a 2-base deletion, window 8)
    for k, word in ((-1, "one base before"), (0, "exactly at"), (1, "one base behind")):
        # the window of round 1 covers reference columns beg_pos .. beg_pos + 7; the tract starts at beg_pos + 1
        n = 7 + k
        name = f"doubling_window_end{k:+d}"
        rng = _rng(name)
        a, b = rand_seq(rng, 300), rand_seq(rng, 300)
        tract = ("AC" * 8)[:n]
        if a[-1] == "C":
            a = a[:-1] + "G"
        nxt = "AC"[n % 2]
        if b[0] == nxt:
            b = other(b[0], 2 if other(b[0]) == nxt else 1) + b[1:]
        ctg = a + tract + b
        out.append(_mk(name, "doubling", f"a 2-base deletion at the start of a {n}-base dinucleotide tract that ends {word} the last column of the first forward window",
                       ctg, [[dele(ctg, 300, 2)]], calls=3))
    # the shortest tract whose forward side is re-issued, and the one a base shorter, by the restated reach
    name = "doubling_first_reissue"
    rng = _rng(name)
    a, b = rand_seq(rng, 300), rand_seq(rng, 300)
    a = a[:-1] + ("G" if a[-1] in "AC" else a[-1])
    b = ("T" if b[0] in "AC" else b[0]) + b[1:]
    calls = {}
    for n in range(2, 16):
        ctg = a + ("AC" * 8)[:n] + b
        v = [dele(ctg, 300, 2)]
        calls[n] = side_rounds(ctg, v, DEFAULT, cluster_score(ctg, v, DEFAULT), False)
    n2 = min(n for n in calls if calls[n] == 2)
    for n, word in ((n2 - 1, "longest tract with one forward call"), (n2, "shortest tract with two")):
        ctg = a + ("AC" * 8)[:n] + b
        out.append(_mk(f"doubling_reissue_{calls[n]}", "doubling", f"a 2-base deletion at the start of a {n}-base dinucleotide tract: the {word}", ctg, [[dele(ctg, 300, 2)]],
                       rounds={0: (1, calls[n])}, calls=1 + calls[n]))
    c("doubling_into_pos0", "a 2-base deletion 40 bases into a dinucleotide tract that starts at position 0: the reverse side doubles until beg_pos == 0",
      "AC", 30, 20, "del", 0, 400, calls=7)
    c("doubling_into_end", "a 2-base deletion in a dinucleotide tract that runs to the contig's last base: the forward side doubles until end_pos == ctg_len",
      "AC", 30, 8, "del", 400, 0, calls=7)
    return out


# ---- diag_*
def _diag_cases():
    out = []
    def mk(name, aim, f, width, **kw):
        r = _rng(name)
        ctg, cls = _spread(r, [(f, width)], lead=500)
        out.append(_mk(name, "diag", aim, ctg, cls, itrs=(1, 2, 4), **kw))
    mk("diag_positive", "deletions of 5 and 3 bases and a SNP in one cluster: main_diag = +8",
       lambda ctg, p: [dele(ctg, p, 5), snp(ctg, p + 8), dele(ctg, p + 12, 3)], 20)
    mk("diag_negative", "insertions of 4 and 3 bases and a SNP in one cluster: main_diag = -7",
       lambda ctg, p, r=_rng("diag_negative_alleles"): [ins(ctg, p, 4, r), snp(ctg, p + 3), ins(ctg, p + 7, 3, r)], 12)
    mk("diag_cancel", "an insertion of 6 bases and a deletion of 6 bases, 5 bases apart: main_diag = 0 with the stop far from either end",
       lambda ctg, p, r=_rng("diag_cancel_alleles"): [ins(ctg, p, 6, r), dele(ctg, p + 5, 6)], 16)
    # an SV-sized insertion: the longest generated query of the table, global scratch
    r = _rng("diag_sv_insertion")
    ctg = rand_seq(r, 2400)
    out.append(_mk("diag_sv_insertion", "diag", "one insertion of 2 000 bases in the middle of a 2 400-base contig: two global-scratch reach jobs whose windows the contig cuts on either side, generated queries of 3 200 bases, main_diag = -2000",
                   ctg, [[ins(ctg, 1200, 2000, r)]]))
    return out


# ---- merge_*
# Found by search (dense random haplotypes over tandem-rich contigs, 2 000 seeds, shrunk variant by variant while the iteration
# count held): a merged cluster's score pays for a longer wander through the tracts around it, which reaches the next neighbour
# only in the following iteration.  In unique sequence a merged cluster reaches no further than its members did.
_MERGE3 = ("CCCCCCCCCAAAAAAAAAAAAAAAAAAAAAAAAAAAAGAGAGAGAGAGAGAGAGAGAGAGAGAGACCGCCGCCGCCGCCGCCGGCGCGATGGCGCCACCCGGTACAATAGATTCCATCAACGAACGAACGAACGAACGAACGAACGAACGGACGGACAGAGCACGAAGGATA"
           "TATATATATATATATACACACACACACACACACACACACACACTAGTATAGTCCCATACGTCTATAGAACTGGCAGAATAAGCATTACACAGT",
           [(120, S, "C", "T"), (142, D, "A", ""), (145, S, "G", "A")])
_MERGE4 = ("ATATATATATCGCACGCACGCACGCACGCACGCACGCACGCACGCACGCACGCACGCACGCACGCAGGGGGGCGGCGGCGGCGGCGGCGGCGGCGGACAGACAGACAGACAGACAGACAGACAGACAGACAGACAGACAGACAGACAGAAGAAGAAGAAGAAGAAGAAGAAGAAGAAGAAGA"
           "ACTTAATGCCACCCCAATTTAGCTCTCTCTCTGGGGGAGAGAGAGAGAGAGAGCGCGCGCGTCTCTCTCCGCGCGTAGGTTTTCTCTTAGAGAAGCATATATATCCATCCGTAAGACTTCAGG",
           [(120, I, "", "G"), (145, D, "C", ""), (152, S, "A", "T"), (185, S, "T", "A")])


def _merge_cases():
    out = []
    rng = _rng("merge_one")
    ctg = rand_seq(rng, 400)
    two = [snp(ctg, 200), snp(ctg, 208)]
    for name, ctg, v, its, n_it in (("merge_one", ctg, two, {1: 1, 2: 2, 4: 2}, "one"), ("merge_two", _MERGE3[0], _MERGE3[1], {1: 1, 2: 2, 4: 3}, "two"),
                                    ("merge_three", _MERGE4[0], _MERGE4[1], {1: 1, 2: 2, 4: 4}, "three")):
        for p, t, r, a in v:
            assert ctg[p:p + len(r)] == r
        out.append(Case(name, "merge", f"{len(v)} variants that take {n_it} merging iteration{'s' if n_it != 'one' else ''} and one more to settle: "
                        f"{', '.join(f'{k} -> {i}' for k, i in its.items())} iterations by limit", ctg, list(v), DEFAULT, (1, 2, 4),
                        dict(iterations=its, clusters=[[0, len(v)]])))
    return out


# ---- edge_*
def _edge_cases():
    out = []
    rng = _rng("edge")
    ctg = rand_seq(rng, 400)
    out.append(_mk("edge_pos1", "edge", "a SNP at position 1: beg_pos = 0 from the start, the reverse side ends after one call", ctg, [[snp(ctg, 1)]], calls=2))
    out.append(_mk("edge_del_pos1", "edge", "a 3-base deletion at position 1", ctg, [[dele(ctg, 1, 3)]], calls=2))
    n = len(ctg)
    out.append(_mk("edge_region_end", "edge", "a SNP on the last base but one: the cluster's region ends at ctg_len", ctg, [[snp(ctg, n - 2)]], calls=2))
    out.append(_mk("edge_del_region_end", "edge", "a 3-base deletion whose region ends at ctg_len", ctg, [[dele(ctg, n - 4, 3)]], calls=2))
    out.append(_mk("edge_both_ends", "edge", "variants at position 1 and next to the last base on a 40-base contig: every window is cut on both sides",
                   ctg[:40], [[snp(ctg, 1)], [snp(ctg[:40], 38)]], calls=4))
    out.append(_mk("edge_last_base", "edge", "a SNP on the last base: the region passes the contig's end by one base, generate_str stops at the end",
                   ctg, [[snp(ctg, n - 1)]], last_base=True, calls=2))
    out.append(_mk("edge_pos0", "edge", "a SNP at position 0: the region starts in front of the contig", ctg, [[snp(ctg, 0)]], undefined="pos0"))
    return out


def _table():
    return _bucket_cases() + _stride_cases() + _ring_cases() + _doubling_cases() + _diag_cases() + _merge_cases() + _edge_cases()


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}
GROUPS = ("bucket", "stride", "ring", "doubling", "diag", "merge", "edge")
assert len(BY_NAME) == len(TABLE)


def fixture_sets():
    """{(pen, iteration limit): [cases]} -- one reference fixture each (the arguments are per fixture); a case of undefined input
    (a variant at position 0, which the reference refuses) is a fixture of its own"""
    out = {}
    for c in TABLE:
        if c.declare.get("undefined"):
            continue
        for it in c.itrs:
            out.setdefault((c.pen, it), []).append(c)
    return out


def fixture_name(pen, it):
    return f"cluster_biwfa_edges_{pen[0]}{pen[1]}{pen[2]}_i{it}"


UNDEFINED = [c for c in TABLE if c.declare.get("undefined")]
