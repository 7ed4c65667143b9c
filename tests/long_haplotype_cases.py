"""Cases behind a haplotype longer than 65 536 bases: the fallback section-edit-distance kernels and the 16-bit borders.

deferred_edit_distances() (pr_api.hip) takes `ed_max_len`, the longest reference / truth haplotype of the BATCH; above
EDB_MAX_TEXT (65 536) every deferred section of the batch leaves k_ed_bits for k_ed_wf, k_ed_diag or the row sweep k_ed.  The long
haplotype can therefore be a supercluster of its own, the `ballast`: one SNP, query equal to truth, nothing deferred.  The sections
under test live in the small superclusters of tests/section_ed_cases.py, whose ref_ed has a reference that needs no oracle: lev(X, Y).

This module holds the ballast, a banded DP that is exact whenever it answers (lev_banded), the selection arithmetic restated
(select), the table of groups, and the spacer cases for the 16-bit borders of the alignment levels.  Nothing here touches a GPU, the
library or the oracle; tests/test_long_haplotype_cases.py shows on the CPU that the table is what it claims,
tests/test_gpu_long_haplotype.py runs it through the kernels."""
from collections import namedtuple

import numpy as np

import section_ed_cases as SC

TYPE_SUB = 1                    # include/vcfdist_pr.h (asserted against the ABI in tests/test_long_haplotype_cases.py)
EDB_MAX_TEXT = 65536            # pr_ed.hip
LDS_LIMIT = 150 * 1024          # 153 600: the selection's bound on both LDS sizes
BALLAST_MARGIN = 50             # contig bases on either side of the ballast's region


# ----------------------------------------------------------------------------------------------------------------------
# the ballast
# ----------------------------------------------------------------------------------------------------------------------
def ballast(n, ctg=0, seed=77):
    """-> (contig, supercluster): the region beg .. end (both inclusive: Lr = end - beg + 1) holds n reference bases and one SNP
    mid-way, the same on both query and both truth haplotypes, so Lq1 == Lq2 == Lt1 == Lt2 == Lr == n (a substitution changes no
    length).  One section of one base each: inline, no deferred job of its own."""
    rng = np.random.RandomState(seed)
    contig = SC._rand(rng, n + 2 * BALLAST_MARGIN)
    p = BALLAST_MARGIN + n // 2
    alt = SC._other(rng, contig[p])
    snp = [(p, TYPE_SUB, chr(contig[p]), chr(alt), 40.0)]
    sc = dict(ctg=ctg, beg=BALLAST_MARGIN, end=BALLAST_MARGIN + n - 1, vars=[snp, snp, snp, snp])
    return contig.decode(), sc


# ----------------------------------------------------------------------------------------------------------------------
# the banded reference
# ----------------------------------------------------------------------------------------------------------------------
def lev_banded(a: bytes, b: bytes, k: int) -> int:
    """Levenshtein distance by the row DP of section_ed_cases.lev restricted to the cells |i - j| <= k; raises ValueError unless the
    result is <= k.

    Why a result <= k is exact.  Every cell of the band holds the cost of SOME edit path (cells outside count as unreachable), so the
    banded result B is an upper bound of the distance D: D <= B.  A path that visits a cell (i, j) has made at least |i - j| insertions
    or deletions by then, so a path of cost <= k never leaves the band.  If B <= k then D <= k, an optimal path lies inside the band,
    the banded DP sees it, and B <= D.  Hence B == D.

    Row i keeps D[i][j] for j = i - k .. i + k at offset j - (i - k); b is padded so that the bases under a row are one slice."""
    n, m = len(a), len(b)
    if abs(n - m) > k:
        raise ValueError(f"lengths {n} and {m} differ by more than the band {k}")
    INF = np.int64(1) << 40
    W = 2 * k + 1
    off = np.arange(W, dtype=np.int64)
    bpad = np.full(max(n, m) + 2 * (k + 1), 255, np.uint8)             # b[j - 1] of row i, offset o (j = i - k + o) is bpad[i + o]
    bpad[k + 1:k + 1 + m] = np.frombuffer(b, np.uint8)
    j = off - k
    prev = np.where((j >= 0) & (j <= m), j, INF)
    up = np.empty(W, np.int64)
    for i, ai in enumerate(a, 1):
        j = off + (i - k)
        up[:-1] = prev[1:] + 1                                  # D[i-1][j] sits one offset to the right in the row above
        up[-1] = INF
        cand = np.minimum(up, prev + (bpad[i:i + W] != ai))     # D[i-1][j-1] sits at the same offset
        cand[(j < 0) | (j > m)] = INF
        prev = np.minimum.accumulate(cand - off) + off          # the horizontal move, as in lev
        prev[(j < 0) | (j > m)] = INF
    d = int(prev[m - (n - k)])
    if d > k:
        raise ValueError(f"banded distance {d} exceeds the band {k}: not proven exact")
    return d


# ----------------------------------------------------------------------------------------------------------------------
# the selection, restated (deferred_edit_distances(), pr_api.hip)
# ----------------------------------------------------------------------------------------------------------------------
def job_lens_same(X: bytes, Y: bytes):
    """(ref_len, tru_len) of the deferred job of a section made by build(mode="same") with both strings non-empty: the section is
    X / Y plus ONE flank base, the matching base behind the insertion (asserted against the oracle's sections on every such case the
    oracle can take, tests/test_long_haplotype_cases.py)"""
    return len(X) + 1, len(Y) + 1


def lds_wf(long_, sum_):
    """bytes of k_ed_wf: two rows of 2 * long + 3 furthest-reaching points of 16 bits, both strings, 16 spare"""
    return 2 * (2 * long_ + 3) * 2 + sum_ + 16


def lds_diag(short, sum_):
    """bytes of k_ed_diag: three diagonals of `pitch` 16-bit cells, both strings, 16 spare"""
    pitch = (short + 2 + 7) & ~7
    return 3 * pitch * 2 + sum_ + 16


def select(jobs, ed_max_len):
    """jobs: [(ref_len, tru_len)] of a batch's deferred sections; ed_max_len: the batch's longest reference / truth haplotype.
    -> (kernel, launches): k_ed_bits up to EDB_MAX_TEXT; beyond it k_ed_wf (a launch per size class: the jobs sorted by their longer
    string, a class ends where 4 * longer <= the class's first) if the batch's largest rows fit LDS and its longest string is below
    29 000; else k_ed_diag if its diagonals fit and the largest sum is below 65 000; else the row sweep k_ed (one slice: the tables
    here stay far below the 2^28 ints of a slice)."""
    if not jobs:
        return None, 0
    if ed_max_len <= EDB_MAX_TEXT:
        return "k_ed_bits", 1
    max_long = max(max(j) for j in jobs)
    max_short = max(min(j) for j in jobs)
    max_sum = max(sum(j) for j in jobs)
    if lds_wf(max_long, max_sum) <= LDS_LIMIT and max_long < 29000:
        longer = sorted((max(j) for j in jobs), reverse=True)
        n_cls, k0 = 0, 0
        while k0 < len(longer):
            k1 = k0
            while k1 < len(longer) and longer[k1] * 4 > longer[k0]:
                k1 += 1
            n_cls += 1
            k0 = k1
        return "k_ed_wf", n_cls
    if lds_diag(max_short, max_sum) <= LDS_LIMIT and max_sum < 65000:
        return "k_ed_diag", 1
    return "k_ed", 1


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
# Lengths are POST-TRIM (nx, ny) = (reference side, truth side), strings unlike at both ends (nothing is trimmed), as in
# section_ed_cases.  A job carries one flank base more on each side (job_lens_same), and the selection counts job lengths:
#   L = nx + 1, S = ny + 1, lds_wf = 8 L + 12 + (L + S) + 16, lds_diag = 6 * pitch(S) + (L + S) + 16, limit 153 600.
#
# cases: the group's cases, one supercluster each; batches: how they are split into batches (index lists; one batch unless given);
# kernels: the kernel expected per batch when a ballast of 65 537 bases follows; ballast: False for the group that runs without one;
# no_oracle: the cases the CPU oracle is not asked about.  It keeps dense (Lq + Lr) x Lt matrices (0.8 to 4.3 G cells for truth
# haplotypes of 19 000 to 65 000 bases: a minute and tens of GB), and its own section distance is the reference's wf_ed, O(d^2)
# in the distance d: measured 3.9 s at d = 17 000, 21 s at 39 700, 55 s at 64 400.  So everything above 17 100 bases is left to
# lev / lev_banded, to status 0, to all-TP, and to the bit-identical run without the ballast, which goes through k_ed_bits: two
# kernels of different construction and a plain DP agree.  The other cases of the same batch keep their oracle parity.
Group = namedtuple("Group", "cases batches kernels ballast no_oracle")


def _group(cases, kernels, batches=None, ballast=True, no_oracle=()):
    batches = batches if batches is not None else (tuple(range(len(cases))),)
    kernels = kernels if isinstance(kernels, tuple) else (kernels,) * len(batches)
    assert len(kernels) == len(batches)
    return Group(tuple(cases), tuple(batches), kernels, ballast, frozenset(no_oracle))


def _smalls(seed):
    """one_group's small shapes (same mode): nx = 63, 64, 65, 127, 128 put x <= nx on the 64-lane tile edges of k_ed, and give
    k_ed_diag jobs far below the launch's max_short"""
    out = []
    for m in (63, 64, 65, 127, 128):
        out += [SC._rr(m, 40, seed, "same"), SC._rr(m, m, seed + 1, "same"), SC._rr(m - 1, m, seed + 2, "same", y="mut")]
        seed += 3
    return out


def _trims():
    """(257, 0), (0, 257), sub_ends, the homopolymer and the two tails of empty_and_trim, query equal to truth"""
    keep = ("del257", "ins257", "sub_ends", "homopolymer", "x_plus_tail", "x_minus_tail")
    return [c for c in SC.GROUPS["empty_and_trim"] if c.mode == "same" and c.name[:-len("_same")] in keep]


def _tile_gaps(seed):
    """k_ed sweeps a row in tiles of 64 lanes over the LONGER string and hands the running minimum of the horizontal move from tile
    to tile (`carry`).  Two cells next to each other differ by at most one, so a row sweep that drops the carry is off by at most one
    per cell, and random strings leave enough slack for the final distance to come out right anyway (seen: such a kernel passed
    every random pair of this table).  These pairs have no slack: the longer string has ONE base more, exactly where lane 63 hands
    over to lane 0 (the step from x = 64 k - 1 to x = 64 k consumes the base of index 64 k - 1), unlike both neighbours so that the
    gap cannot move; distance 1, or 2 for two such bases.  On the reference side and on the truth side."""
    out = []
    for n, at in ((300, (63,)), (300, (127,)), (300, (255,)), (300, (63, 191)), (8000, (6399,))):
        name = f"n{n}_at{'_'.join(map(str, at))}"
        lo, hi = at[0], at[-1]
        out.append(SC._one(f"x_minus_{name}", ("rand", n), ("x-bases", at), seed, "same", (hi - lo + 1, hi - lo + 1 - len(at))))
        at_y = tuple(i - k for k, i in enumerate(at))           # (the k-th extra base sits k places further right in the longer string)
        out.append(SC._one(f"x_plus_{name}", ("rand", n), ("x+bases", at_y), seed + 1, "same", (at_y[-1] - lo, at_y[-1] - lo + len(at))))
        seed += 2
    return out


def _planted(n, seed, mode="same", k=196):
    # Y = X with 196 planted edits, then both ends made unlike: at most 198 <= 200 edits, inside lev_banded's k = 400
    return SC._one(f"rand{n}_planted{n}_{mode}", ("rand", n), ("planted", n, k), seed, mode, (n, n))


PLANTED_K = 400

GROUPS = {
    # 33 to 8 193 bases: L = 8 194 and the largest sum 8 193 + 4 201 give lds_wf = 65 552 + 12 + 12 394 + 16 < 153 600, L < 29 000.
    # Size classes (x 4 apart, by the longer string): from 8 194, from 2 001, from 129 or so: at least three launches with an LDS
    # size each (test_long_haplotype_cases.py counts them from the job lengths).
    "wf_classes": _group(SC.GROUPS["one_group"] + SC.GROUPS["multi_group"], "k_ed_wf"),
    # the last batch k_ed_wf takes and the first it does not:
    #   (17 000, 40): L = 17 001, S = 41: 136 008 + 12 + 17 042 + 16 = 153 078 <= 153 600
    #   (17 100, 40): L = 17 101, S = 41: 136 808 + 12 + 17 142 + 16 = 153 978 >  153 600; lds_diag = 6 * 48 + 17 142 + 16: k_ed_diag
    "wf_diag_border": _group([SC._rr(17000, 40, 6000, "same"), SC._rr(17100, 40, 6001, "same")], ("k_ed_wf", "k_ed_diag"),
                             batches=((0,), (1,))),
    # 16-bit distances: (40 000, 300) random strings are at least 39 700 apart, above 32 767, on either side.  The largest sum
    # k_ed_diag takes is 64 999 = 64 698 + 301, i.e. post-trim (64 697, 300) (the issue's (64 699, 300) less the two flank bases).
    # pitch(301) = 304: lds_diag = 1 824 + 64 999 + 16; lds_wf is far beyond.  The smalls ride in the same launch.
    "diag_u16": _group([SC._rr(40000, 300, 6100, "same"), SC._rr(300, 40000, 6102, "same"), SC._rr(64697, 300, 6101, "same")]
                       + _smalls(6110), "k_ed_diag", no_oracle=(0, 1, 2)),
    # the first sum k_ed_diag refuses: 65 000 = 64 699 + 301, post-trim (64 698, 300), on either side: the row sweep.  With the
    # smalls, the trims and the one-base gaps on the tile edges (_tile_gaps).
    "row_sweep": _group([SC._rr(64698, 300, 6200, "same"), SC._rr(300, 64698, 6201, "same")] + _smalls(6210) + _trims()
                        + _tile_gaps(6250), "k_ed", no_oracle=(0, 1)),
    # the other route into k_ed: L = S = 19 301: lds_wf = 154 408 + 12 + 38 602 + 16 and lds_diag = 6 * 19 304 + 38 602 + 16 = 154 442
    # both exceed 153 600 while the sum, 38 602, is far below 65 000.
    "row_sweep_square": _group([SC._rr(19300, 19300, 6300, "same", y="mut")], "k_ed", no_oracle=(0,)),
    # k_ed_bits with its planes nearly full, WITHOUT ballast: text of 65 001 columns (plane words up to index 2 031), pattern of
    # 65 001 rows = 16 groups of 4 096.  The supercluster is the section plus 2 * SC_MARGIN + 1 = 65 201 (65 301) bases <= 65 536.
    # Reference: lev_banded(k = 400) alone.
    #   mode `same` (cases 0, 1): REFUSED.  The query haplotype then carries the 65 000-base deletion and insertion itself; its
    #     alignments are too long for one workgroup, and the strip planner (k_strip_plan, pr_strip.hip) finds no column within
    #     ST_CAP = 4 088 of a cut where QUERY and REF map 1:1, so all four come back with VPR_ST_ERR_LIMIT and no variant results.
    #     That refusal is what is asserted, and that the other supercluster of the batch is untouched by it.
    #   mode `fn` (cases 3, 4): the query has no variant, its haplotypes are the reference; the alignment distance is lev(X, Y) and
    #     both truth variants are false negatives with ref_ed == query_ed == lev(X, Y) (the oracle on twins of 300 and 1 500 bases,
    #     tests/test_long_haplotype_cases.py).  Each alone, and each behind a `packed` case in one batch (stale planes).
    "bits_full_planes": _group([_planted(65000, 6400), _planted(65100, 6401), SC.GROUPS["packed"][1],
                                _planted(65000, 6400, "fn"), _planted(65100, 6401, "fn")], "k_ed_bits",
                               batches=((3,), (4,), (2, 3), (2, 4), (0,), (2, 1)), ballast=False, no_oracle=(0, 1, 2, 3, 4)),
}
BITS_REFUSED = frozenset((0, 1))        # cases of bits_full_planes whose four alignments carry VPR_ST_ERR_LIMIT
# selection_edge: `packed` followed by ballast(65 536): k_ed_bits; by ballast(65 537): k_ed_wf (33 to 258 bases)
SELECTION_EDGE = ("packed", ((65536, "k_ed_bits"), (65537, "k_ed_wf")))
BALLAST_LEN = 65537


def expected_distance(case, X, Y):
    """the reference of one pair: lev_banded for the planted cases (a full lev of 65 000 x 65 000 takes minutes), lev otherwise"""
    if case.pairs[0][1][0] == "planted":
        return lev_banded(X, Y, PLANTED_K)
    return SC.lev(X, Y)


# ----------------------------------------------------------------------------------------------------------------------
# spacer cases: the 16-bit borders of the alignment levels
# ----------------------------------------------------------------------------------------------------------------------
# One supercluster = [cluster left] + n variant-free random bases + [cluster right].  The clusters are a few FP / FN SNPs and
# small indels (total alignment distance far below 16: nothing beyond the 256-cell window is needed), different on the two query
# and on the two truth haplotypes so that the phase matters.  Everything the library answers for it must not depend on n: the
# answer for n = 300, which the oracle gives in milliseconds, is the answer at Lt = 64 999 .. 65 537 (ZL_MAXLEN 65 000 of pr_zl.hip,
# the 0xffff pointer field of the lane words, d.Lt > 0xfffe in the planner, the 0xffff sort key).
SPACER_MARGIN = 60
CLUSTER_LEN = 40
# a cluster: per hap slot (query 1, query 2, truth 1, truth 2) a list of (offset in the cluster, kind, length);
# kind "snp" | "ins" | "del"; the bases come from the case's seed, the same for every slot at the same offset
CLUSTERS = {
    "A": ([(5, "snp", 1), (20, "snp", 1), (28, "ins", 2)],              # query 1: TP, FP, TP
          [(5, "snp", 1), (28, "ins", 2)],                              # query 2
          [(5, "snp", 1), (12, "snp", 1), (28, "ins", 2)],              # truth 1: TP, FN, TP
          [(5, "snp", 1), (12, "snp", 1)]),                             # truth 2: no insertion
    "B": ([(6, "del", 2), (15, "snp", 1), (22, "snp", 1)],              # query 1: a deletion one base short, FP, TP
          [(6, "del", 3)],                                              # query 2
          [(6, "del", 3), (22, "snp", 1)],                              # truth 1
          [(6, "del", 3), (22, "snp", 1), (30, "ins", 1)]),             # truth 2
    "C": ([(3, "ins", 3), (18, "snp", 1)],
          [(3, "ins", 3), (18, "snp", 1), (33, "del", 1)],
          [(3, "ins", 2), (18, "snp", 1)],
          [(18, "snp", 1), (25, "snp", 1)]),
}
SPACER_LT = (64999, 65000, 65001, 65534, 65535, 65536, 65537)
# one pair per entry of SPACER_LT (the i-th with seed i), chosen among those for which the oracle raises no VPR_ST_SWAP_TIE: a tie
# replay numbers (Lq + Lr + 2 Lt) * Lt cells with 32 bits, and the library refuses the whole call (VPR_ERR_ARG) for an alignment
# with a tie beyond that, about 32 767 bases.  SPACER_TIE is such a case (cluster C's two insertions of 3 and 2 bases at one
# position): its refusal is asserted on its own.
SPACER_PAIRS = (("A", "B"), ("B", "A"), ("C", "A"), ("C", "B"), ("C", "B"), ("C", "A"), ("B", "C"))
SPACER_TIE = ("A", "C", 0)              # (left, right, seed)


def _cluster_vars(rng, contig, at, cluster):
    """the four slots' variant lists of one cluster placed at contig position `at`; -> (vars[4], truth-1 length change)"""
    alts = {}
    out = []
    for slot in cluster:
        vs = []
        for off, kind, ln in slot:
            p = at + off
            if (off, kind, ln) not in alts:
                alts[(off, kind, ln)] = (chr(SC._other(rng, contig[p])) if kind == "snp" else SC._rand(rng, ln).decode())
            if kind == "snp":
                vs.append((p, TYPE_SUB, chr(contig[p]), alts[(off, kind, ln)], 40.0))
            elif kind == "ins":
                vs.append((p, SC.TYPE_INS, "", alts[(off, kind, ln)], 40.0))
            else:
                vs.append((p, SC.TYPE_DEL, contig[p:p + ln].decode(), "", 40.0))
        out.append(vs)
    delta = sum(ln if kind == "ins" else -ln if kind == "del" else 0 for _, kind, ln in cluster[2])
    return out, delta


def spacer_case(k_left, k_right, n, ctg=0, seed=0):
    """-> (contig, supercluster, Lt of truth haplotype 1): margin + cluster + n random bases + cluster + margin; the region covers
    all of it but 10 contig bases on either side.  The clusters' bases do not depend on n (drawn before the spacer)."""
    rng = np.random.RandomState(9000 + seed)
    head = SC._rand(rng, 10 + SPACER_MARGIN + CLUSTER_LEN)
    tail = SC._rand(rng, CLUSTER_LEN + SPACER_MARGIN + 10)
    seeds = rng.randint(0, 1 << 30, 2)
    contig = head + SC._rand(np.random.RandomState(rng.randint(0, 1 << 30)), n) + tail
    at_l, at_r = 10 + SPACER_MARGIN, len(head) + n
    vl, dl = _cluster_vars(np.random.RandomState(seeds[0]), contig, at_l, CLUSTERS[k_left])
    vr, dr = _cluster_vars(np.random.RandomState(seeds[1]), contig, at_r, CLUSTERS[k_right])
    beg, end = 10, len(contig) - 10
    sc = dict(ctg=ctg, beg=beg, end=end, vars=[vl[h] + vr[h] for h in range(4)])
    return contig.decode(), sc, end - beg + 1 + dl + dr


def spacer_n(k_left, k_right, lt, seed=0):
    """the spacer length at which truth haplotype 1 of spacer_case(k_left, k_right, n) has lt bases"""
    return lt - spacer_case(k_left, k_right, 0, seed=seed)[2]


def spacer_batch(lts=SPACER_LT, n=None):
    """-> (contigs, superclusters, lts): one supercluster per entry of SPACER_PAIRS, the i-th with truth haplotype 1 of lts[i] bases,
    or (n given) all with a spacer of n bases: the twins"""
    contigs, scs, got = [], [], []
    for i, (kl, kr) in enumerate(SPACER_PAIRS):
        c, sc, lt = spacer_case(kl, kr, n if n is not None else spacer_n(kl, kr, lts[i]), ctg=i, seed=i)
        contigs.append(c); scs.append(sc); got.append(lt)
    return contigs, scs, got


ALN_COLUMNS = ("aln_dist", "aln_end_plane", "aln_beg_plane", "aln_status")
SC_COLUMNS = ("sc_phase", "orig_phase_dist", "swap_phase_dist")
VAR_COLUMNS = ("errtype", "sync_group", "credit", "ref_ed", "query_ed", "callq")


def result_columns(res, var_off, first=0, count=None):
    """every array compare() of test_gpu_parity.py looks at, restricted to the superclusters first .. first + count - 1 of a batch
    with the variant offsets var_off[hap slot]: {name: array}; floats as their bit patterns.  The spacer rule lives here: the
    oracle's answer for a spacer case is the SAME in every one of these arrays whatever the spacer's length (sync_group counts a
    supercluster's groups, not positions), so a long supercluster is held to its short twin by plain equality of these columns."""
    count = res.n_sc - first if count is None else count
    out = {}
    for f in ALN_COLUMNS:
        out[f] = np.asarray(getattr(res, f))[4 * first:4 * (first + count)].copy()
    for f in SC_COLUMNS:
        out[f] = np.asarray(getattr(res, f))[first:first + count].copy()
    for f in VAR_COLUMNS:
        for h in range(4):
            lo, hi = int(var_off[h][first]), int(var_off[h][first + count])
            for w in range(2):
                a = np.asarray(getattr(res, f)[h][w])[lo:hi]
                out[f, h, w] = (a.view(np.uint32) if a.dtype == np.float32 else a).copy()
    return out


def differing_columns(a, b):
    """names of the columns of two result_columns() dicts that are not bit-identical (with the first differing indices)"""
    assert sorted(map(str, a)) == sorted(map(str, b))
    return [(k, np.flatnonzero(a[k] != b[k])[:8].tolist() if a[k].shape == b[k].shape else (a[k].shape, b[k].shape))
            for k in a if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]
