"""Alignments whose optimal path runs along the EDGE of a window level, for pinning the exit test of the window ladder
(k_fwd_q16, k_fwd_stripe, k_fwd_wide<4>, k_fwd_wide<16>: 16 / 64 / 256 / 1024 cells per plane; exit_key / exit_lb, pr_band.hip).

The construction: a tandem tract unit * reps (unit a random primitive u-mer) between random flanks.  The truth carries an insertion
of `unit` at the tract's start and the query one at its end (deletion form: deletions of one unit), so the two haplotype strings
are IDENTICAL while their pointers differ: the optimal path runs for the whole tract on a diagonal exactly u cells off the centre
r2q[t2r[t]] the windows follow.  Swapping the callsets gives the other sign.  Truth-only SNPs in a flank price the case (s = 1, 2,
3); k point mutations inside the tract (written into the contig: only variants are ever variants) make the shifted path cost 2k
against the u of the in-window alternative, with a container-order tie at 2k == u.

This module holds the case builders, the table, a restatement in numpy of every level's window origins (written from the kernels'
text: stripe_origin, wide_origin<W>, the origin lambda of pr_q16.hip, query_center, k_prep_tj) and of exit_end, and needed_level():
the smallest level whose restated windows hold every cell on an optimal path (the cells the oracle's backward sweep scored, and
its path).  The exit test's bound is D(b) + cost(edge) + LB(c -> end): exit_min > s says that no path from the origin to an END
cell of cost <= s leaves the window, so those cells are what a level must hold and no level below needed_level may accept.
(It says nothing of a cell with D <= s from which the end is further than s - D away: the forward expansion of a case with s > 0
reaches such cells all along the tract, one diagonal further out, and a window that cuts them is still exact -- the backward sweep
never comes there.  `level_fwd`, the level that would hold all the cells the forward expansion reached, is kept beside `level` as
a figure: shift_w64_u29+del_s1b needs 64 cells and 256 for its forward reach, the 64-cell level accepts it, rightly.)
It imports no product code beyond _abi; tests/test_window_edge_cases.py shows on the CPU that the table is what it claims and that
every border of every level is covered from both sides, tests/test_gpu_window_edges.py runs it through the kernels."""
import zlib
from collections import namedtuple

import numpy as np

import oracle_lib as O
from vcfdist_amd import _abi as A

_BASES = np.frombuffer(b"ACGT", np.uint8)
PAD = 30                # contig bases outside the region, on either side (0 on a side the case cuts at the contig's end)
FLANK = 40              # default length of the region's leading / trailing flank
LEVELS = (16, 64, 256, 1024)
DENSE = 1 << 20         # the "level" of an alignment no window holds
STRIPE_ROWS = {16: 4, 64: 8, 256: 8, 1024: 8}      # Q_K, FS_K, WD_K, WD_K


def next_level(W):
    return DENSE if W == LEVELS[-1] else LEVELS[LEVELS.index(W) + 1]


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
# family: shift | priced | there_back | phase | plane_end | short | slack | het | het_same | slide | swap
#      het: the query's second haplotype is the reference (its alignments are slides, below: they need the level the shifted ones
#      need, both have to hold offset u); het_same: it carries the truth's own variant, so its alignments run along the centre and
#      the four alignments of the supercluster need different levels
#      swap: a slide with a query-only insertion (qn bases, qat bases into the tract).  A REF-plane cell at offset <= u whose
#      position lies behind the insertion while the row's centre lies in front of it changes planes, at no cost, into a QUERY-plane
#      cell qn further out: optimal cells that only a swap edge reaches (along the QUERY plane they lie behind qn inserted bases).
#      Chosen among 396 candidates as those that a build without the swap key, or with a bound one too high, accepted too low
#      (scratch builds; profiles/README.md has the runs)
#      slide: the truth's variant alone, the query is the reference: distance u, and every placement of the unit inside the tract is
#      optimal, so the optimal cells fill the offsets 0 .. u (deletion form: -u .. 0) -- and with no query variant every budget
#      of the exit test is zero: its bound is exact there, exit_min == s for the level that cuts an optimal cell
# W: the level whose edge the case is aimed at (a label: what it needs is computed, never declared)
# u: unit length; sign +1: the truth's variant in front (the path runs ABOVE the centre in the query plane), -1: callsets swapped
# form: "ins" | "del"; snp: truth-only SNPs, side "front" | "back" flank; k: point mutations inside the tract
# lead / tail: flank lengths inside the region; reps: units in the tract; het: the query's variant on its first haplotype only
# cut: "" | "del_end" / "qdel_end": the contig ends with the region and a truth-only / query-only deletion takes its last three
#      bases, so the planes do not end on the truth's last reference base (exit_end's slack is 3)
# dist: the declared distance of alignment (query 1, truth 1); tie: all four alignments carry ST_SWAP_TIE (2k == u, sign +1; with
#      the callsets swapped the oracle's path changes planes behind the mutations for free and it reports no tie)
Case = namedtuple("Case", "name family W u sign form snp side k lead tail reps het cut dist tie qn qat")
Built = namedtuple("Built", "case contig sc tract0")       # tract0: where the (first) tract begins in the contig


def _case(family, W, u, sign, form="ins", snp=0, side="front", k=0, lead=FLANK, tail=FLANK, reps=None, het=False, cut="", qn=0, qat=0):
    if reps is None:
        reps = 3 if u >= 16 else -(-48 // u)
        if k > 1:
            reps = max(reps, 6)
    dist = snp + (min(u, 2 * k) if k else 0) + (u if family in ("slide", "swap") else 0) + (3 if cut == "del_end" else 0)     # (a query-only deletion is free: the REF plane)
    name = f"{family}_w{W}_u{u}{'+' if sign > 0 else '-'}{form}_s{snp}{side[0]}_k{k}_l{lead}_t{tail}_r{reps}{'_het' if het else ''}{'_' + cut if cut else ''}{f'_q{qn}at{qat}' if qn else ''}"
    return Case(name, family, W, u, sign, form, snp, side, k, lead, tail, reps, het, cut, dist, bool(k) and 2 * k == u and sign > 0, qn, qat)


def _rand(rng, n):
    return bytearray(rng.choice(_BASES, n).tobytes())


def _other(rng, *avoid):
    return int(rng.choice([c for c in b"ACGT" if c not in avoid]))


def _unit(rng, u):
    """a random primitive u-mer: no rotation of it but the trivial one equals it"""
    while True:
        s = bytes(_rand(rng, u))
        if u == 1 or (s + s).find(s, 1) == u:
            return bytearray(s)


def _tract(rng, u, reps, k, before):
    """-> (unit, tract): unit * reps with k point mutations at k different offsets inside the unit (so that no two are a multiple
    of u apart), spread over the units but the first and the last;
    the unit's last base differs from `before`, the base in front of the tract, so the shift cannot slide out of it"""
    while True:
        unit = _unit(rng, u)
        if unit[-1] != before:
            break
    tract = unit * reps
    for i, m in enumerate(sorted(rng.choice(u, k, replace=False)) if k else ()):
        at = (1 + i * (reps - 2) // k) * u + int(m)
        tract[at] = _other(rng, tract[at])
    return unit, tract


def _shift_variants(p0, unit, tract, form):
    """-> (front, back): the variant at the tract's start and the one at its end that leave the same string"""
    u, p1 = len(unit), p0 + len(tract)
    if form == "ins":
        return (p0, A.TYPE_INS, "", unit.decode(), 40.0), (p1, A.TYPE_INS, "", unit.decode(), 30.0)
    return (p0, A.TYPE_DEL, tract[:u].decode(), "", 40.0), (p1 - u, A.TYPE_DEL, tract[len(tract) - u:].decode(), "", 30.0)


def build(case, ctg=0):
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    c = case
    contig = _rand(rng, PAD) + _rand(rng, c.lead)
    beg = PAD
    t, q = [], []
    n_tracts = 2 if c.family == "there_back" else 1
    tract0 = len(contig)
    for i in range(n_tracts):
        if i:
            contig += _rand(rng, 30)
        unit, tract = _tract(rng, c.u, c.reps, c.k, contig[-1] if contig else 0)
        p0 = len(contig)
        contig += tract
        front, back = _shift_variants(p0, unit, tract, c.form)
        first_in_truth = (c.sign > 0) == (i == 0)          # the second tract of there_back shifts the other way
        (t if first_in_truth else q).append(front)
        if c.family not in ("slide", "swap"):
            (q if first_in_truth else t).append(back)
        if c.qn > 0:        # a query-only insertion of qn random bases / deletion of -qn bases, qat bases into the tract
            q.append((p0 + c.qat, A.TYPE_INS, "", _rand(rng, c.qn).decode(), 20.0))
        elif c.qn < 0:
            q.append((p0 + c.qat, A.TYPE_DEL, tract[c.qat:c.qat - c.qn].decode(), "", 20.0))
    t_shift = list(t)
    tail = _rand(rng, c.tail)
    if tail and tail[0] == unit[0]:
        tail[0] = _other(rng, unit[0])
    contig += tail
    end = len(contig)
    sc_end = end
    if c.cut == "del_end":              # the contig ends with the region, and a truth-only deletion takes its last three bases
        t.append((end - 3, A.TYPE_DEL, contig[end - 3:end].decode(), "", 40.0))
        sc_end = end + 1
    elif c.cut == "qdel_end":
        q.append((end - 3, A.TYPE_DEL, contig[end - 3:end].decode(), "", 40.0))
        sc_end = end + 1
    else:
        contig += _rand(rng, PAD)
    # truth-only SNPs, 7 bases apart, from the flank's far end
    for j in range(c.snp):
        p = (beg + 3 + 7 * j) if c.side == "front" else (end - 4 - 7 * j)
        assert (p < tract0) if c.side == "front" else (p >= end - c.tail), case.name
        t.append((p, A.TYPE_SUB, chr(contig[p]), chr(_other(rng, contig[p])), 40.0))
    t.sort()
    q.sort()
    sc = dict(ctg=ctg, beg=beg, end=sc_end, vars=[q, (sorted(t_shift) if c.family == "het_same" else []) if c.het else q, t, t])
    return Built(case, contig.decode(), sc, tract0)


def batch_of(cases):
    """one batch, a contig and a supercluster per case -> (Variants, Batch, [Built])"""
    built = [build(c, ctg=i) for i, c in enumerate(cases)]
    v = A.Variants.from_sites([b.contig for b in built], [b.sc for b in built])
    return v, O.generate(v), built


# ----------------------------------------------------------------------------------------------------------------------
# the window origins of each level, restated
# ----------------------------------------------------------------------------------------------------------------------
def tj_of(t2r, tflag):
    """k_prep_tj: the offset of truth position t inside its run of equal pointers (a truth insertion), 0 outside a variant"""
    t2r = np.asarray(t2r, np.int64)
    same = np.zeros(len(t2r), bool)
    same[1:] = (t2r[1:] == t2r[:-1]) & ((np.asarray(tflag[1:]) & A.PTR_VARIANT) != 0)
    first = np.searchsorted(t2r, t2r, side="left")
    return np.where(same, np.minimum(np.arange(len(t2r)) - first, 65535), 0)


def query_center(t2r, tj, r2q, t, Lr):
    """query_center (pr_band.hip): the query position of t's reference base, plus t's offset inside a truth insertion as far as
    the query hap inserts bases there too"""
    r = min(max(int(t2r[t]), 0), Lr - 1)
    q = int(r2q[r])
    j = int(tj[t])
    if j == 0:
        return q
    kq = int(r2q[r + 1]) - q - 1 if r + 1 < Lr else 0
    return q + min(j, max(kq, 0))


def _cdiv2(a):
    return int(a / 2)           # C's division truncates towards zero


def origins(W, t2r, tj, r2q, Lq, Lr):
    """-> (loQ[stripe], loR[stripe]) of level W: constant over stripes of STRIPE_ROWS[W] truth rows, centred between the reference
    (query) coordinates of the stripe's first and last row, clamped to the plane, stripe 0 at the origin"""
    K, Lt = STRIPE_ROWS[W], len(t2r)
    n = (Lt + K - 1) // K
    loQ, loR = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for s in range(1, n):
        ta, tb = s * K, min(s * K + K - 1, Lt - 1)
        ra, rb = int(t2r[ta]), int(t2r[tb])
        qa, qb = query_center(t2r, tj, r2q, ta, Lr), query_center(t2r, tj, r2q, tb, Lr)
        loR[s] = max(0, min(_cdiv2(ra + rb) - W // 2, Lr - min(W, Lr)))
        loQ[s] = max(0, min(_cdiv2(qa + qb) - W // 2, Lq - min(W, Lq)))
    return loQ, loR


def exit_end(q2r, t2r, Lr):
    """exit_end (pr_band.hip) -> (endT, slack): how far the two planes' last positions are from the truth's last reference base"""
    endT = int(t2r[-1])
    return endT, max(abs(int(q2r[-1]) - endT), abs(Lr - 1 - endT))


def arrays_of(batch, sc, aln):
    """-> (q2r, t2r, tflag, r2q, Lq, Lr, Lt) of alignment aln = 2 * query hap + truth hap of supercluster sc"""
    qs, ts = aln >> 1, 2 + (aln & 1)
    qo, to, ro = batch.hap_off[qs], batch.hap_off[ts], batch.ref_off
    q2r = batch.hap_ptr[qs][qo[sc]:qo[sc + 1]]
    t2r = batch.hap_ptr[ts][to[sc]:to[sc + 1]]
    tflag = batch.hap_flag[ts][to[sc]:to[sc + 1]]
    r2q = batch.ref_ptr[qs][ro[sc]:ro[sc + 1]]
    return q2r, t2r, tflag, r2q, len(q2r), len(r2q), len(t2r)


Need = namedtuple("Need", "level level_fwd dist status off_lo off_hi n_cells slack dists statuses lens")


def needed_level(batch, sc, aln):
    """-> Need: the smallest level whose windows hold every cell on an optimal path (scored by the oracle's backward sweep, both
    planes) and its path; level_fwd: the same for every cell the forward expansion reached (non-zero forward flags); the oracle's
    distance and status; the extreme offsets of the path's QUERY-plane cells from the window centre r2q[t2r[t]]; the number of
    cells on optimal paths; exit_end's slack; the four distances, statuses and the lengths of the supercluster.
    (The oracle backtracks from the preferred end plane only: where dist_q == dist_r the optimal paths into the other end cell are
    not scored, and `level` can be lower than what the kernel has to hold -- a weaker pin there, never a wrong one.)"""
    ex = O.Extra(batch, want=(sc, aln), dump_matrices=True)
    res = O.run(batch, extra=ex)
    q2r, t2r, tflag, r2q, Lq, Lr, Lt = arrays_of(batch, sc, aln)
    tj = tj_of(t2r, tflag)
    pl, qri, ti, _, _ = ex.path_arrays()
    def cells_of(mats, keep):
        out = []
        for p in range(2):
            x, t = np.nonzero(keep(mats[p]))
            m = pl == p
            out.append((np.concatenate([x, qri[m]]).astype(np.int64), np.concatenate([t, ti[m]]).astype(np.int64)))
        return out

    def level_holding(cells):
        for W in LEVELS:
            K = STRIPE_ROWS[W]
            lo = origins(W, t2r, tj, r2q, Lq, Lr)
            if all(((x >= lo[p][t // K]) & (x <= np.minimum((Lq, Lr)[p] - 1, lo[p][t // K] + W - 1))).all() for p, (x, t) in enumerate(cells)):
                return W
        return DENSE

    cells = cells_of(ex.pscore, lambda m: m >= 0)
    level = level_holding(cells)
    level_fwd = level_holding(cells_of(ex.flags, lambda m: m != 0))
    mq = pl == A.PLANE_QUERY
    ctr = np.asarray(r2q, np.int64)[np.clip(np.asarray(t2r, np.int64)[ti[mq]], 0, Lr - 1)]
    off = qri[mq].astype(np.int64) - ctr
    return Need(level, level_fwd, int(res.aln_dist[4 * sc + aln]), int(res.aln_status[4 * sc + aln]), int(off.min()) if len(off) else 0,
                int(off.max()) if len(off) else 0, int(sum(len(x) for x, _ in cells)), exit_end(q2r, t2r, Lr)[1],
                tuple(int(d) for d in res.aln_dist[4 * sc:4 * sc + 4]), tuple(int(d) for d in res.aln_status[4 * sc:4 * sc + 4]),
                tuple(batch.lens(sc)))


def _needs_of(case):
    _, batch, _ = batch_of([case])
    # (a homozygous case's four alignments are the same problem four times)
    return case.name, [needed_level(batch, 0, aln) for aln in ((0, 1, 2, 3) if case.het else (0,))]


_NEEDS = {}


def needs(cases):
    """{case name: [Need per alignment]} (one entry for a homozygous case), computed once per process, on up to eight cores"""
    todo = [c for c in cases if c.name not in _NEEDS]
    if todo:
        import multiprocessing
        import os
        import sys
        n = max(1, min(8, len(os.sched_getaffinity(0)), len(todo) // 4))
        if not os.path.exists(getattr(sys.modules.get("__main__"), "__file__", None) or ""):
            n = 1           # (a spawned worker re-imports __main__: not from a script read from standard input)
        if n > 1:
            O.lib()         # (built once, in the parent)
            # (fresh interpreters, not forks: the GPU tests call this from a process that has the device open)
            with multiprocessing.get_context("spawn").Pool(n) as pool:
                _NEEDS.update(pool.map(_needs_of, todo, chunksize=4))
        else:
            _NEEDS.update(map(_needs_of, todo))
    return {c.name: _NEEDS[c.name] for c in cases}


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
def _sweep(W):
    return [u for u in range(W // 2 - 10, W // 2 + 3) if u >= 1]


def _table():
    out = []
    for W in LEVELS:
        for sign in (1, -1):
            for u in _sweep(W):
                out.append(_case("shift", W, u, sign))                               # distance 0
                out.append(_case("priced", W, u, sign, k=1))                         # distance min(u, 2)
            for u in _sweep(W)[4:]:
                out.append(_case("shift", W, u, sign, form="del", snp=1, side="back"))
                out.append(_case("shift", W, u, sign, snp=2, side="front"))
            out.append(_case("shift", W, W // 2 - 2, sign, snp=3, side="back"))
            out.append(_case("shift", W, W // 2 - 2, sign, form="del"))
    # 2k in {u - 2, u, u + 2}: the tie and its two neighbours.  (With the callsets swapped the oracle's distance at u >= 26 is
    # below min(u, 2k) -- the path leaves the shifted diagonal for the other plane between the mutations -- so those are sign +1 only.)
    # At u >= 26 the tie and 2k = u + 2 only: with 2k = u - 2 a path that mixes the two routes is cheaper than either.
    for u, signs in ((4, (1, -1)), (8, (1, -1)), (26, (1,)), (28, (1,)), (30, (1,))):
        for sign in signs:
            for k in (u // 2 - 1, u // 2, u // 2 + 1)[u >= 26:]:
                if k == 1:
                    continue            # (in the sweep above)
                out.append(_case("priced", 16 if u < 16 else 64, u, sign, k=k))
    for W, u in ((16, 6), (64, 26), (256, 122)):
        for sign in (1, -1):
            out.append(_case("there_back", W, u, sign))
            for extra in (0, 3, 7):
                out.append(_case("phase", W, u, sign, lead=FLANK + extra))
            out.append(_case("het", W, u, sign, het=True))
            out.append(_case("het", W, u, sign, het=True, snp=1, side="back"))
            for du in (2, 6):       # (u + 6: the shifted alignments need the next level)
                out.append(_case("het_same", W, u + du, sign, het=True))
                out.append(_case("het_same", W, u + du, sign, het=True, snp=1, side="back"))
        for d in (1, 2, W // 2):        # (0: a variant on the region's last / first base is no legal input)
            out.append(_case("plane_end", W, u, 1, tail=d))
            out.append(_case("plane_end", W, u, -1, lead=d))
    for W in (16, 64, 256):
        for u in range(W // 2 - 3, W // 2 + 3):
            out.append(_case("slide", W, u, 1))
            out.append(_case("slide", W, u, 1, form="del"))
    # the 1024-cell level's own acceptance (distance u >= 509 costs the oracle: two units, short flanks, the deletion form only:
    # planes of 1 043 bases, 2 s each): 509 needs 1024 cells, 510 the dense sweep
    for u in (509, 510):
        out.append(_case("slide", 1024, u, 1, form="del", reps=2, lead=12, tail=12))
    # the same two families AT the border: the last unit length that fits and the first that does not (sign +1 / -1)
    for W, edge in ((16, {1: 5, -1: 7}), (64, {1: 27, -1: 29}), (256, {1: 123, -1: 125})):
        for sign in (1, -1):
            for u in (edge[sign], edge[sign] + 1):
                if (W, u, sign) == (16, 6, 1):
                    continue            # (the cases above)
                for extra in (0, 3, 7):
                    out.append(_case("phase", W, u, sign, lead=FLANK + extra))
                for d in (1, 2):
                    out.append(_case("plane_end", W, u, sign, **({"tail": d} if sign > 0 else {"lead": d})))
    for W, u, form, reps, qn, qat in ((64, 8, "ins", 13, 26, 24), (64, 8, "ins", 13, 26, 48), (64, 8, "ins", 13, 28, 24), (64, 8, "ins", 13, 28, 48),
                                      (64, 8, "ins", 13, 30, 24), (64, 8, "ins", 13, 30, 48), (64, 2, "del", 52, 28, 26), (64, 2, "del", 52, 30, 26),
                                      (64, 3, "del", 35, 28, 51), (64, 3, "ins", 35, 60, 24), (64, 5, "del", 21, 26, 25), (256, 3, "del", 99, 118, 72),
                                      (256, 3, "del", 99, 126, 147), (256, 8, "del", 37, 160, 72), (256, 8, "ins", 37, 118, 144)):
        out.append(_case("swap", W, u, 1, form=form, reps=reps, qn=qn, qat=qat))
    for n in (1, 2, 5, 11, 13):         # planes shorter than the window: haplotypes of 5 to 70 bases
        out.append(_case("short", 16 if n < 11 else 64, n, 1, lead=2, tail=2, reps=4))
        out.append(_case("short", 16 if n < 11 else 64, n, -1, form="del", lead=2, tail=2, reps=4))
    for W, u in ((16, 6), (64, 26)):
        for sign in (1, -1):
            for cut in ("del_end", "qdel_end"):
                out.append(_case("slack", W, u, sign, cut=cut))
    return out


TABLE = _table()
