"""python -m vcfdist_amd <query.vcf[.gz]> <truth.vcf[.gz]> <ref.fasta[.gz]> [-b regions.bed] [options]

The reference's command line for the precision/recall evaluation (vcfdist v2.6.4, main.cpp / globals.cpp) on top of
the MI355X path: VCF / BED / FASTA readers (include/vcfdist_io.h), biWFA or distance clustering and superclustering
(include/vcfdist_cluster.h), the precision/recall alignment on the GPU (include/vcfdist_pr.h), phasing, counters and
the PRECISION-RECALL SUMMARY and the output tables (include/vcfdist_report.h: precision-recall*.tsv, phase-blocks.tsv,
superclusters.tsv, query.tsv, truth.tsv, summary.vcf under -p PREFIX; -n writes nothing).  With -d the alignment-distance
metrics run on the GPU behind each contig's path (include/vcfdist_distance.h): distance.tsv, distance-summary.tsv, edits.tsv and
the ALIGNMENT DISTANCE SUMMARY (printed even with -n); one rank only.  With -rq / -rt a callset is clustered and realigned on the
GPU before the evaluation (include/vcfdist_realign.h): orig-query.vcf / orig-truth.vcf as read, query.vcf / truth.vcf realigned;
-ro stops after the realignment; one rank only.  With --stratify FILE (the GIAB list format: one name<TAB>path of a BED per line) the
counters of the one evaluation are also cut by region on the GPU (include/vcfdist_strata.h): stratified-precision-recall.tsv and
stratified-precision-recall-summary.tsv; works under several ranks in both --shard modes.  With --stratify-context the default
sequence-context strata (include/vcfdist_context.h: intervals built on the GPU from the FASTA) follow the list's strata, or stand
alone, and context-strata.bed holds their intervals.  With --stratify-repeats the default repeat strata (include/vcfdist_repeats.h:
where the FASTA is not unique, found genome-wide on the GPU before the contig loop) follow the list's strata, in front of the context
strata, and repeat-strata.bed holds their intervals.  With --stratify-long-repeats the default long repeat strata (repeated 64-, 100-
and 250-mers, include/vcfdist_longrepeats.h: one more genome-wide pass) follow those, and long-repeat-strata.bed holds their intervals.
With --stratify-near-repeats K:M[,K:M...] the near-repeat strata the user names (k-mers that occur again within M substitutions,
include/vcfdist_nearrepeats.h: one more genome-wide pass) follow those, and near-repeat-strata.bed holds their intervals.
With --stratify-variants the default variant strata
(include/vcfdist_varstrata.h: transitions / transversions, indel size bins, hom / het, isolated / crowded -- bits made on the GPU from
the variant tables) follow those, or stand alone, and variant-strata.tsv lists them with their numbers of members.  With
--stratify-derive NAME=EXPR (repeatable) a stratum is made on the GPU from the membership bits of the strata in front of it
(include/vcfdist_derive.h: & | ! and parentheses over stratum names, '*' globs standing for the union of what they match), and with
--stratify-cross LIST:LIST (repeatable) every pair a&b of the two lists of globs; they follow every other stratum, the derived ones
first, need another --stratify* option, and derived-strata.tsv lists them with their numbers of members.  With --bootstrap N
the counters are
resampled N times on the GPU (include/vcfdist_bootstrap.h: a Poisson bootstrap over superclusters, conditional on the phasing, the
BEST threshold kept at the point estimate's): bootstrap-precision-recall-summary.tsv with 95 % percentile intervals for precision,
recall and F1, bootstrap-replicates.tsv, and with --stratify stratified-bootstrap-precision-recall-summary.tsv; --bootstrap-seed S
(default 1); works under several ranks in both --shard modes.  With --classify-errors every query FP and truth FN gets the first
error class that applies (include/vcfdist_errclass.h: the right allele with the wrong genotype, on the aligned or on the other
haplotype, another allele at the site, something within --error-window N bases (default 50), nothing), joined across the callsets on
the GPU: error-classes.tsv and error-classes-summary.tsv; works under several ranks in both --shard modes.  With --cut-classes
(beside a --classify-* option and a --stratify* option or --bootstrap) the label counts are cut by the strata and resampled as
well (include/vcfdist_labelcut.h): stratified-error-classes*.tsv, bootstrap-error-classes-summary.tsv and the match-kinds
counterparts; works under several ranks in both --shard modes.  With --classify-matches
every TP of either callset gets the first match kind that applies (include/vcfdist_matchkind.h: exact -- what an allele-for-allele
comparison finds --, shifted, regrouped, partial), from the resident sync groups on the GPU: match-kinds.tsv and
match-kinds-summary.tsv; works under several ranks in both --shard modes."""
import argparse
import os
import re
import sys
from dataclasses import dataclass, field

import numpy as np

from . import _abi as A
from . import api, cluster as K, io as IO, report as RP, summary as S


def transfer_phase_sets(slots, clusters, sc):
    """superclusterData::transfer_phase_sets (cluster.cpp:186-330): one phase set per supercluster from the variants' PS.
    The reference walks the superclusters, inside one the four haps (query 1, 2, truth 1, 2) and their variants, keeps one
    running maximum of PS per callset, and a variant whose PS exceeds its callset's maximum makes its PS the current phase
    set; a supercluster gets the phase set current at its end.  Only a variant whose PS exceeds every PS in front of it on
    its own hap can do that, so the walk is done over those few candidates (numpy finds them) instead of all variants."""
    first_pos, phase_set = None, 0
    for s in slots:
        nz = np.nonzero(s["phase_set"])[0]
        if len(nz) and (first_pos is None or s["pos"][nz[0]] < first_pos):
            first_pos, phase_set = int(s["pos"][nz[0]]), int(s["phase_set"][nz[0]])
    cand = []
    for i, s in enumerate(slots):
        off = sc.var_off(i)
        n = int(off[-1]) if len(off) else 0
        if n == 0:
            continue
        ps = np.asarray(s["phase_set"][:n], dtype=np.int64)
        run = np.maximum.accumulate(ps)
        idx = np.nonzero((ps != 0) & (ps > np.concatenate(([0], run[:-1]))))[0]
        sc_of = np.searchsorted(off, idx, side="right") - 1
        cand += [(int(k), i, int(v), int(ps[v])) for v, k in zip(idx, sc_of)]
    cand.sort()                                   # processing order: supercluster, hap slot, variant
    cur = [0, 0]
    ev_k, ev_v = [], []
    for k, i, v, ps in cand:
        if ps > cur[i >> 1]:
            cur[i >> 1] = ps
            ev_k.append(k); ev_v.append(ps)
    out = np.full(sc.n, phase_set, np.int32)
    if ev_k:
        ek, ev = np.asarray(ev_k), np.asarray(ev_v, dtype=np.int32)
        last = np.searchsorted(ek, np.arange(sc.n), side="right") - 1      # last update at or before each supercluster
        out = np.where(last >= 0, ev[np.maximum(last, 0)], phase_set).astype(np.int32)
    return out


WARN_TEXT = (       # dist.cpp:1203-1223, raised per alignment as VPR_ST_WARN_* bits
    (A.ST_WARN_REF_ED, "Nonzero reference edit distance with no truth variants at ctg %s supercluster %d"),
    (A.ST_WARN_QUERY_ED, "Query edit distance changed with no query variants at ctg %s supercluster %d"),
    (A.ST_WARN_EXCEEDS, "Query edit distance exceeds reference edit distance at ctg %s supercluster %d"),
    (A.ST_WARN_ZERO_ED, "Zero edit distance with truth variants at ctg %s supercluster %d"),
)


ERR_TEXT = ((A.ST_ERR_LIMIT, "exceeds an implementation limit of the GPU path (more than eight swap sources on one position, or an alignment "
                             "the dense kernels cannot place)"),
            (A.ST_ERR_NO_PTR, "ended in a walk without a path pointer"), (A.ST_ERR_UNFINISHED, "was left unfinished"))


def print_warnings(name, aln_status, strict=False):
    """the reference's WARN lines for the conditions calc_prec_recall flags (one line per alignment and condition), and -- LOUDLY --
    the alignments this implementation did NOT evaluate (VPR_ST_ERR_*: the reference has no such limits and evaluates them).
    Their variants stay ERRTYPE_UN and are missing from the counts; their superclusters' phasing is taken from what was
    evaluated.  -> number of superclusters with such an alignment; with strict the run ends instead (--strict)."""
    for bit, text in WARN_TEXT:
        for a in np.nonzero(aln_status & np.uint32(bit))[0]:
            print("[WARN  vcfdist] " + text % (name, int(a) // 4), file=sys.stderr)
    bad_sc = set()
    for bit, text in ERR_TEXT:
        idx = np.nonzero(aln_status & np.uint32(bit))[0]
        if len(idx) == 0:
            continue
        scs = sorted({int(a) // 4 for a in idx})
        bad_sc.update(scs)
        print(f"[WARN  vcfdist_amd] contig '{name}': {len(idx)} alignment(s) in {len(scs)} supercluster(s) {text}: NOT EVALUATED -- their variants are "
              f"left out of every count and table (superclusters {', '.join(map(str, scs[:12]))}{' ...' if len(scs) > 12 else ''})", file=sys.stderr)
    if bad_sc and strict:
        raise SystemExit(f"ERROR: contig '{name}': {len(bad_sc)} supercluster(s) not evaluated (--strict)")
    return len(bad_sc)


def cluster_hap(s, seq, args, device):
    """a hap's columns as a K.HapSeq, and its clusters as the run clusters: biWFA on the GPU, or by gap / size"""
    h = K.HapSeq.__new__(K.HapSeq)
    K.Hap.__init__(h, s["pos"], s["rlen"], s["type"], s["ref_len"], s["alt_len"])
    h.ref_off, h.alt_off, h.pool = s["ref_off"], s["alt_off"], s["pool"]
    if args.cluster == "biwfa":
        return h, K.wfa_cluster(h, bytes(seq), sub=args.sub, open=args.open, extend=args.extend, max_cluster_itrs=args.max_iterations,
                                reach_min_gap=args.reach_min_gap, device=device)[0]
    return h, K.simple_cluster(h, 1 if args.cluster == "size" else 0, args.cluster_gap, args.reach_min_gap)


def prepare_contig(name, seq, slots, args, device=0):
    """everything in front of the precision/recall path for one contig: clustering, superclustering and the host
    marshalling (generate_ptrs_strs).  A contig the library cannot marshal (vpr_batch_from_variants, include/vcfdist_pr.h)
    raises here, before any contig has been evaluated."""
    haps, cl = map(list, zip(*(cluster_hap(s, seq, args, device) for s in slots)))
    sc = K.supercluster(haps, cl, args.max_supercluster_size)
    batch = None
    if sc.n:
        v = A.Variants(np.array([0, len(seq)], np.int64), seq, np.zeros(sc.n, np.int32), sc.beg, sc.end,
                       [sc.var_off(i) for i in range(4)], [h.pos for h in haps], [h.type for h in haps],
                       [s["var_qual"] for s in slots], [h.ref_off for h in haps], [h.ref_len for h in haps],
                       [h.alt_off for h in haps], [h.alt_len for h in haps], [h.pool for h in haps])
        batch = api.batch_from_variants(v)
    return dict(name=name, haps=haps, cl=cl, sc=sc, batch=batch, slots=slots, variants=v if sc.n else None)


# The families of default strata, in the order of their strata behind the list's: their option, their word in the messages and their
# defaults; the genome-wide k-mer families (include/vcfdist_repeats.h, include/vcfdist_longrepeats.h) also name api.PrecisionRecall's
# methods for their pass and report's writer of their BED
FAMILIES = (
    dict(option="--stratify-repeats", word="repeat", defaults=api.repeats_default, intervals="repeat_intervals",
         download="download_repeat_intervals", stats_call="repeat_stats", timing="repeat_timing", write="write_repeat_bed"),
    dict(option="--stratify-long-repeats", word="long repeat", defaults=api.longrepeats_default, intervals="longrepeat_intervals",
         download="download_longrepeat_intervals", stats_call="longrepeat_stats", timing="longrepeat_timing", write="write_long_repeat_bed"),
    dict(option="--stratify-context", word="sequence-context", defaults=api.context_default),
    dict(option="--stratify-variants", word="variant", defaults=api.varstrata_default),
)


def option_on(args, option):
    return getattr(args, option[2:].replace("-", "_"))


# The near-repeat family (include/vcfdist_nearrepeats.h) has no defaults: its strata are the user's, parsed from the option's value
NEAR_OPTION = "--stratify-near-repeats"
NEAR_FAMILY = dict(option=NEAR_OPTION, word="near repeat", defaults=None, intervals="nearrepeat_intervals",
                   download="download_nearrepeat_intervals", stats_call="nearrepeat_stats", stats_kw=dict(cost=True), timing="nearrepeat_timing",
                   write="write_near_repeat_bed")


def near_strata(text):
    """the value of --stratify-near-repeats, K:M[,K:M...] -> [A.VprNearStratum]; the messages are main.cpp's"""
    specs = []
    for entry in text.split(","):
        m = re.fullmatch(r"([0-9]{1,9}):([0-9]{1,9})", entry)
        if m is None:
            raise SystemExit(f"ERROR: {NEAR_OPTION}: entry '{entry}' is not K:M")
        k, mm = int(m.group(1)), int(m.group(2))
        if mm > A.NREP_MAX_M or k < 8 * (mm + 1) or k > A.NREP_MAX_K:
            raise SystemExit(f"ERROR: {NEAR_OPTION}: entry '{entry}': M must be 0 to {A.NREP_MAX_M} and K 8 (M + 1) to {A.NREP_MAX_K}")
        if any((sp.k, sp.m) == (k, mm) for sp in specs):
            raise SystemExit(f"ERROR: {NEAR_OPTION}: duplicate entry '{entry}'")
        if len(specs) == A.NREP_MAX_SPEC:
            raise SystemExit(f"ERROR: {NEAR_OPTION}: more than {A.NREP_MAX_SPEC} entries")
        specs.append(A.near_kmer(k, mm))
    return specs


def stratifying(args):
    return bool(args.stratify) or bool(args.stratify_near_repeats) or any(option_on(args, row["option"]) for row in FAMILIES)


@dataclass
class Family:
    """a row of FAMILIES in a StrataPlan, and what the run makes of it"""
    option: str; word: str; defaults: object
    intervals: str = None; download: str = None; stats_call: str = None; timing: str = None; write: str = None
    stats_kw: dict = field(default_factory=dict)    # the near-repeat family: its statistics with the cost
    specs: object = None                            # the strata's parameters; None: the option is off
    names: list = field(default_factory=list)
    rows: dict = field(default_factory=dict)        # k-mer families, context: per contig, every stratum's intervals
    stats: object = None                            # k-mer families: the valid and the repeated starts of every stratum (near: and the cost)
    ms: float = 0.0                                 # on the device


@dataclass
class Derived:
    """the derived and the crossed strata of a StrataPlan (--stratify-derive, --stratify-cross; include/vcfdist_derive.h), behind every
    other stratum: their names, kinds (A.DV_KIND_*) and expressions as derived-strata.tsv lists them, and the one call's programs"""
    names: list = field(default_factory=list)
    kinds: list = field(default_factory=list)
    expressions: list = field(default_factory=list)
    code_off: list = field(default_factory=lambda: [0])
    code: list = field(default_factory=list)
    ms: float = 0.0                                 # on the device

    def add(self, name, kind, expression, code):
        self.names.append(name); self.kinds.append(kind); self.expressions.append(expression)
        self.code += [int(c) for c in code]
        self.code_off.append(len(self.code))


@dataclass
class StrataPlan:
    """which strata, in which order (StrataPlan in main.cpp): every stratum's name in table order, the list's BEDs, the families"""
    names: list = field(default_factory=list)
    beds: list = field(default_factory=list)
    families: list = field(default_factory=lambda: [Family(**row) for row in FAMILIES])
    near: Family = field(default_factory=lambda: Family(**NEAR_FAMILY))     # the user's near-repeat strata, behind the long repeat family's
    derived: Derived = field(default_factory=Derived)                       # behind everything else
    kmer = property(lambda self: [fam for fam in self.families[:2] + [self.near] if fam.specs])       # the genome-wide families that are on
    ordered = property(lambda self: self.families[:2] + [self.near] + self.families[2:])            # in table order
    ctx = property(lambda self: self.families[2])
    vs = property(lambda self: self.families[3])


@dataclass
class LabelPass:
    """--classify-errors / --classify-matches (LabelPass in main.cpp): the names of api.PrecisionRecall's methods and of report's
    writers (looked up when they are called), the pass's stderr line, and its sums over the contigs"""
    noun: str; labels: int; label: str; timing: str; cut_strata: str; cut_boot: str; cut_timing: str
    write: str; write_strata: str; write_boot: str; line: object
    extra: tuple = ()                               # arguments of `label` behind the phasing
    counts: object = None; strata: object = None; boot: object = None      # [2][4][labels][nq]; --cut-classes: per stratum, per replicate
    ms: float = 0.0; cut_ms: float = 0.0


def errclass_line(p):
    return (f"[vcfdist_amd] error classes: window {p.extra[0]}, {int(p.counts[0, 3, :, 0].sum())} query FP and "
            f"{int(p.counts[1, 3, :, 0].sum())} truth FN classified, {p.ms:.3f} ms on the device")


def matchkind_line(p):
    qk, tk = p.counts[0, 3, :, 0], p.counts[1, 3, :, 0]
    return (f"[vcfdist_amd] match kinds: query TP {int(qk[0])} exact, {int(qk[1])} shifted, {int(qk[2])} regrouped, {int(qk[3])} partial; "
            f"truth TP {int(tk[0])} exact, {int(tk[1])} shifted, {int(tk[2])} regrouped, {int(tk[3])} partial, {p.ms:.3f} ms on the device")


class Totals:
    """the sums over the contigs (Totals in main.cpp): counts[2][4][3][nq], with strata the stratified ones, the hap-variants seen
    and in no stratum and the variant strata's members per callset (behind everything else the derived strata's, when there are
    such), with --bootstrap the replicates' (and per stratum), the label
    passes with their cuts.  tally lists the int64 arrays that are summed over the ranks, in the order of the vector (pack, unpack):
    every sum is added in place, so the list made here stays the owners'."""
    def __init__(self, args, plan):
        nq = args.max_qual - args.min_qual + 1
        n_strata, n_rep = len(plan.names) if plan else 0, args.bootstrap
        zeros = lambda *shape: np.zeros(shape, np.int64)
        self.total = zeros(2, 4, 3, nq)
        self.strat = zeros(n_strata, 2, 4, 3, nq) if plan else None
        self.seen_none = zeros(2) if plan else None
        self.vs_members = zeros(2, len(plan.vs.specs or ())) if plan else None
        self.boot = zeros(n_rep, 2, 4, 3, nq) if n_rep else None
        self.boot_strat = zeros(n_strata, n_rep, 2, 4, 3, nq) if n_rep and plan else None
        self.boot_ms = 0.0
        self.passes = []        # in the order of their counts in the vector, of their files and of their stderr lines
        if args.classify_errors:
            window = A.EC_DEFAULT_WINDOW if args.error_window is None else args.error_window
            self.passes.append(LabelPass("error classes", A.EC_CLASSES, "errclass", "errclass_timing", "errclass_strata", "errclass_boot",
                                         "errclass_cut_timing", "write_error_classes", "write_error_classes_stratified",
                                         "write_error_classes_bootstrap", errclass_line, (window,)))
        if args.classify_matches:
            self.passes.append(LabelPass("match kinds", A.MK_KINDS, "matchkind", "matchkind_timing", "matchkind_strata", "matchkind_boot",
                                         "matchkind_cut_timing", "write_match_kinds", "write_match_kinds_stratified",
                                         "write_match_kinds_bootstrap", matchkind_line))
        for p in self.passes:
            p.counts = zeros(2, 4, p.labels, nq)
            if args.cut_classes:
                p.strata = zeros(n_strata, 2, 4, p.labels, nq) if plan else None
                p.boot = zeros(n_rep, 2, 4, p.labels, nq) if n_rep else None
        tally = [self.total, self.strat, self.seen_none, self.vs_members, self.boot, self.boot_strat] + [p.counts for p in self.passes]
        self.dv_members = zeros(2, len(plan.derived.names)) if plan and plan.derived.names else None
        self.tally = [a for a in tally + [cut for p in self.passes for cut in (p.strata, p.boot)] + [self.dv_members] if a is not None]


def pack(arrays):
    """the vector the ranks sum: the arrays of a tally one behind the other"""
    return np.concatenate([a.ravel() for a in arrays])


def unpack(arrays, vector):
    """the summed vector back into the arrays it was packed from"""
    at = 0
    for a in arrays:
        a[...] = vector[at:at + a.size].reshape(a.shape)
        at += a.size


def stratify_contig(pr, prep, plan, tot, args, pb, part_idx=None):
    """--stratify*: the contig's membership words on the device (every hap-variant against every stratum), then the counters of the
    executed batch cut by them, added to tot.strat.  part_idx: this rank holds the superclusters part_idx of the contig -- the
    words are computed for the whole contig and the rank keeps its share's."""
    from . import shard
    name, whole = prep["name"], prep["batch"]
    n_strata = len(plan.names)
    # the interval table: the rows of --stratify's BEDs, with --stratify-repeats and --stratify-long-repeats the contig's rows of the
    # genome-wide passes behind them
    table = None
    if plan.beds or plan.kmer:
        table = A.Strata([[b.intervals(name)] for b in plan.beds] + [[row] for fam in plan.kmer for row in fam.rows[name]], 1)
    if plan.ctx.specs:      # --stratify-context: the context intervals are built on the device and go to the same mask kernel
        pr.context_masks(prep["variants"], plan.ctx.specs, table)
        keep_context_intervals(pr, plan.ctx, name)
    elif table is not None:
        pr.strata_masks(prep["variants"], table)
    dv = plan.derived
    n_vs = len(plan.vs.specs or ())
    n_pre = n_strata - len(dv.names) - n_vs
    if plan.vs.specs:       # --stratify-variants: the bits made from the variant tables follow in the same words
        pr.varstrata_masks(prep["variants"], plan.vs.specs, append=n_pre > 0)
        plan.vs.ms += pr.varstrata_timing()
    if dv.names:            # --stratify-derive, --stratify-cross: one call on the bits that are there, per variant (a shard's edge cannot matter)
        pr.derive_masks(dv.code_off, dv.code)
        dv.ms += pr.derive_timing()
    words = pr.download_strata_masks()
    if part_idx is not None:
        words = [np.stack([shard.subset_per_variant(w, whole.var_off[s], part_idx) for w in words[s]]) for s in range(4)]
        pr.upload_strata_masks(n_strata, words)
    tot.strat += S.pr_counts_strata(pr, None, pb, args.min_qual, args.max_qual)     # (the classes are resident: pr_counts)
    for w in words:
        tot.seen_none += (w.shape[1], int((np.bitwise_or.reduce(w, axis=0) == 0).sum()))
    # variant-strata.tsv, derived-strata.tsv: the members of every variant stratum and of every derived one, per callset
    for members, first, n in ((tot.vs_members, n_pre, n_vs), (tot.dv_members, n_pre + n_vs, len(dv.names))):
        for k in range(first, first + n):
            for s, w in enumerate(words):
                members[s >> 1, k - first] += int(((w[k >> 6] >> np.uint64(k & 63)) & np.uint64(1)).sum())


def keep_context_intervals(pr, ctx, name):
    """the context intervals of the contig the last context_masks saw, for context-strata.bed and the stderr line"""
    ctx.rows[name] = [row[0] for row in pr.download_context_intervals()]
    ctx.ms += pr.context_timing()[0]


def kmer_strata(fam, fasta, args, device=0):
    """--stratify-repeats, --stratify-long-repeats, --stratify-near-repeats: the family's genome-wide pass over all contigs of the FASTA, those without a
    variant included, on a handle of its own that is gone before the evaluation starts.  Every rank computes the same arrays."""
    cfg = A.default_config(device=device)
    cfg.max_qual = float(args.max_qual)
    pr = api.PrecisionRecall(cfg)
    names = list(fasta)
    getattr(pr, fam.intervals)([fasta[c] for c in names], fam.specs)
    rows = getattr(pr, fam.download)()
    fam.rows = {c: [rows[k][j] for k in range(len(fam.specs))] for j, c in enumerate(names)}
    fam.stats = getattr(pr, fam.stats_call)(**fam.stats_kw)
    fam.ms = sum(getattr(pr, fam.timing)())
    pr.close()


def context_only(name, seq, ctx, args, device=0):
    """--stratify-context for a contig (or a rank's share of one) without a supercluster: the intervals alone, for no variant"""
    cfg = A.default_config(device=device)
    cfg.max_qual = float(args.max_qual)
    pr = api.PrecisionRecall(cfg)
    z32, z64, z8 = np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8)
    seq = np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, np.uint8)
    v = A.Variants(np.array([0, len(seq)], np.int64), seq, z32, z32, z32, [z64] * 4, [z32] * 4, [z8] * 4, [np.zeros(0, np.float32)] * 4,
                   [np.zeros(0, np.int64)] * 4, [z32] * 4, [np.zeros(0, np.int64)] * 4, [z32] * 4, [z8] * 4)
    pr.context_masks(v, ctx.specs)
    keep_context_intervals(pr, ctx, name)
    pr.close()


def bootstrap_contig(pr, tot, plan, args, pb, keys):
    """--bootstrap: the replicate counters of the executed batch, added to tot.boot; with strata one pass per stratum of the
    resident membership words, added to tot.boot_strat"""
    kw = dict(n_rep=args.bootstrap, seed=args.bootstrap_seed, min_qual=args.min_qual, max_qual=args.max_qual)
    tot.boot += pr.pr_counts_boot(None, pb, keys, **kw)        # (the classes are resident: pr_counts)
    tot.boot_ms += pr.boot_info()[1]
    if plan is not None:
        for k in range(len(plan.names)):
            tot.boot_strat[k] += pr.pr_counts_boot(None, pb, keys, stratum=k, **kw)
            tot.boot_ms += pr.boot_info()[1]


def label_contig(pr, variants, passes, args, pb):
    """--classify-errors / --classify-matches: the labels of the executed batch by each of `passes`, added to its counts (the variant
    classes are resident: pr_counts)"""
    for p in passes:
        p.counts += getattr(pr, p.label)(variants, None, pb, *p.extra, args.min_qual, args.max_qual)
        p.ms += getattr(pr, p.timing)()


def cut_contig(pr, passes, plan, args, keys):
    """--cut-classes: the label counts of every pass cut by the strata and resampled (include/vcfdist_labelcut.h), behind
    stratify_contig and bootstrap_contig: the label bytes and the share's membership words are both resident.  Added to the
    pass's strata / boot."""
    for p in passes:
        if plan is not None:
            p.strata += getattr(pr, p.cut_strata)(args.min_qual, args.max_qual)
            p.cut_ms += getattr(pr, p.cut_timing)()[0]
        if args.bootstrap:
            p.boot += getattr(pr, p.cut_boot)(keys, args.bootstrap, args.bootstrap_seed, args.min_qual, args.max_qual)
            p.cut_ms += getattr(pr, p.cut_timing)()[1]


@dataclass
class Ranks:
    """this process among the run's: under torch.distributed.run one process per GPU; dist is torch.distributed with its group up, or
    None on one rank; cdev is where the collectives' tensors live (None: the host, gloo); by_sc: --shard superclusters on several ranks"""
    rank: int; world: int; device: int; dist: object = None; cdev: object = None; by_sc: bool = False


def count_contig(pr, prep, args, plan, tot, cls, pb, variants, keys, idx=None):
    """the one counting sequence behind an executed batch: counters, labels, strata, replicates, cuts, each reading what the one
    before left resident.  idx: the superclusters of the contig the handle holds (None: all of them); cls, pb, variants and keys
    are the caller's for that set.  -> counts[2][4][3][nq], everything else added to tot"""
    counts = S.pr_counts(pr, cls, pb, args.min_qual, args.max_qual)
    label_contig(pr, variants, tot.passes, args, pb)
    if plan is not None:
        stratify_contig(pr, prep, plan, tot, args, pb, part_idx=idx)
    if args.bootstrap:
        bootstrap_contig(pr, tot, plan, args, pb, keys)
    if args.cut_classes:
        cut_contig(pr, tot.passes, plan, args, keys)
    return counts


def distance_contig(pr, prep, args, dist_sets):
    """-d: edits_wrapper behind the precision/recall path (main.cpp:223-238), from what it left on the device"""
    d = pr.distance(prep["variants"], eval_sub=args.eval_sub, eval_open=args.eval_open, eval_extend=args.eval_extend,
                    min_qual=args.min_qual, max_qual=args.max_qual)
    info = d["info"]
    if info.n_limit or info.n_error:
        print(f"[WARN  vcfdist_amd] contig '{prep['name']}': {info.n_limit} distance alignment(s) beyond the device's memory plan and "
              f"{info.n_error} that failed: NOT EVALUATED -- left out of the distance metrics", file=sys.stderr)
    print(f"[vcfdist_amd] {prep['name']}: {info.n_jobs} distance alignments, {info.n_edits} edits, edit distance {int(d['qual_dists'].min())}",
          file=sys.stderr)
    dist_sets.append((prep["name"], d))


NOT_EVALUATED = np.uint32(A.ST_ERR_LIMIT | A.ST_ERR_NO_PTR | A.ST_ERR_UNFINISHED)


def mask_unevaluated(r):
    """a supercluster with an alignment the GPU path did not evaluate (VPR_ST_ERR_*): its phase distances come from alignments
    that were cut short -- it takes no side in the contig's phasing (print_warnings reports it)"""
    bad = np.unique(np.nonzero(r.aln_status & NOT_EVALUATED)[0] // 4)
    if len(bad):
        r.sc_phase[bad] = A.PHASE_NONE


def evaluate_contig(prep, args, ranks, plan, tot, dist_sets=None, ordinal=0):
    """the precision/recall path on the GPU, phasing and counters for a prepared contig.  -> int64 counters [2][4][3][nq] and what
    the writers need: (clusters after splitting, superclusters, results, phase sets, pb_phase, switches, flips).
    With ranks.by_sc this rank evaluates its share of the contig's SUPERCLUSTERS -- dealt by the
    reference's own size estimate (shard.deal: LPT + snake, as precision_recall_threads_wrapper spreads superclusters over its
    threads, dist.cpp:1670-1726) -- the per-supercluster phasing is all-gathered (the contig's phasing needs all of it and
    every rank then runs it), the counters returned are this rank's share (the caller all-reduces the sum over the contigs),
    and the result records are gathered (every rank gets the contig's full tables; rank 0 writes them)."""
    name, haps, cl, sc, slots = prep["name"], prep["haps"], prep["cl"], prep["sc"], prep["slots"]
    counts = np.zeros_like(tot.total)
    if sc.n == 0:
        z = np.zeros(0, np.int32)
        return counts, (sc.clusters, sc, A.Results(0, [len(h.pos) for h in haps]), z, z, z, z)
    cfg = A.default_config(device=ranks.device)
    cfg.max_qual = float(args.max_qual); cfg.credit_threshold = args.credit_threshold; cfg.phase_threshold = args.phase_threshold
    pr = api.PrecisionRecall(cfg)
    phase_sets = transfer_phase_sets(slots, cl, sc)
    cls = [S.var_class(h.type, h.ref_len, h.alt_len, args.sv_threshold) for h in haps]
    if not ranks.by_sc:
        res = pr.run(prep["batch"])
        if dist_sets is not None:
            distance_contig(pr, prep, args, dist_sets)
        mask_unevaluated(res)
        pb, sw, fl = S.phase(res.sc_phase, phase_sets)
        counts = count_contig(pr, prep, args, plan, tot, cls, pb, prep["variants"], A.boot_keys(ordinal, np.arange(sc.n)))
    else:
        from . import shard
        whole = prep["batch"]
        idx = shard.deal(shard.estimate_cells(whole), ranks.world)[ranks.rank]
        mine = whole.subset(idx)
        # (every rank enters the collectives below: a rank whose share fails tells the others first, and all end together --
        # a lone SystemExit would leave the rest waiting in all_gather for ever)
        err = None
        try:
            local = pr.run(mine) if len(idx) else A.Results(0, [0, 0, 0, 0])
        except Exception as e:      # noqa: BLE001 -- whatever it is (VprError, MemoryError, OSError ...), the other ranks must hear of it
            err, local = e, None
        if shard.any_rank(err is not None, device=ranks.cdev):
            raise api.VprError(str(err) if err is not None else "another rank's share of the contig failed")
        mask_unevaluated(local)
        sc_phase, _, _ = shard.allgather_phase(local, idx, sc.n, device=ranks.cdev)
        pb, sw, fl = S.phase(sc_phase, phase_sets)
        if len(idx):    # (everything is local to the supercluster, sync groups too: the rank labels its share from its share's tables)
            cls_mine = [shard.subset_per_variant(cls[s], whole.var_off[s], idx) for s in range(4)]
            variants = shard.subset_variants(prep["variants"], idx) if tot.passes else None
            counts = count_contig(pr, prep, args, plan, tot, cls_mine, pb[idx], variants, A.boot_keys(ordinal, idx), idx)
        res = shard.gather_results(local, idx, whole.var_off, device=ranks.cdev)
        if ranks.rank != 0:
            # (--strict ends the run on EVERY rank: the gathered status column is the same everywhere, rank 0 prints the report
            # below and the others leave with it instead of waiting in the next contig's collective -- ADVICE r5)
            if args.strict and (res.aln_status & NOT_EVALUATED).any():
                raise SystemExit(1)
            return counts, (sc.clusters, sc, res, phase_sets, pb, sw, fl)
    print_warnings(name, res.aln_status, strict=args.strict)
    print(f"[vcfdist_amd] {name}: {sum(len(h.pos) for h in haps)} hap-variants, {sum(c.n for c in cl)} clusters, {sc.n} superclusters, "
          f"{len(sw)} switch / {len(fl)} flip errors", file=sys.stderr)
    return counts, (sc.clusters, sc, res, phase_sets, pb, sw, fl)


def check_contigs(q, t, fasta, bed):
    """check_contigs (bed.cpp:135-284) -> the contigs to evaluate, in the order the reference's superclusterData walks them
    (the query's list after the check: its VCF order, then what the check appends).  With a BED only its contigs count
    (others are dropped from both callsets and need not be in the FASTA); without one every truth contig has to be in the
    FASTA."""
    warn = lambda m: print("[WARN  vcfdist] " + m, file=sys.stderr)
    qc, tc = list(q["contigs"]), list(t["contigs"])
    if bed is not None:
        qc = [c for c in qc if c in bed.contigs]
        tc = [c for c in tc if c in bed.contigs]
        for c in qc:
            if c not in tc:
                warn(f"Contig '{c}' found in query VCF but not truth VCF.")
        for c in tc:
            if c not in qc:
                warn(f"Contig '{c}' found in truth VCF but not query VCF.")
        for c in bed.contigs:
            if c not in fasta:
                raise SystemExit(f"ERROR: Contig '{c}' found in BED but not reference FASTA.")
            if c not in qc:
                qc.append(c)
        return qc
    for c in tc:
        if c not in fasta:
            raise SystemExit(f"ERROR: Contig '{c}' found in truth VCF but not reference FASTA. Please provide BED file.")
        if c not in qc:
            warn(f"Contig '{c}' found in truth VCF but not query VCF. All truth variants on '{c}' will be false negatives.")
            qc.append(c)
    for c in qc:
        if c not in tc:
            warn(f"Contig '{c}' found in query VCF but not truth VCF. All query variants on '{c}' will be false positives.")
            if c not in fasta:
                raise SystemExit(f"ERROR: contig '{c}' not in reference FASTA")
    return qc


def realign_callset(which, cs, fasta, args, device=0):
    """wf_swg_realign + left_shift of a whole callset (main.cpp:74-100): per contig and hap, cluster as the run clusters (biWFA on
    the GPU, or gap / size), then vrl_realign.  -> the callset with its hap columns replaced by the realigned ones"""
    out, n_cl, n_in, n_out, kept = [], 0, 0, 0, dict(edge=0, limit=0, error=0)
    for k, ctg in enumerate(cs["contigs"]):
        if ctg not in fasta:
            raise SystemExit(f"ERROR: Contig '{ctg}' not in reference FASTA (realignment of the {which} VCF)")
        seq = fasta[ctg]
        per = []
        for s in cs["vars"][k]:
            cl = cluster_hap(s, seq, args, device)[1]
            try:
                cols, _, info = api.realign(s, cl, seq, sub=args.sub, open=args.open, extend=args.extend, max_qual=args.max_qual, device=device)
            except api.VprError as e:
                raise SystemExit(f"ERROR: contig '{ctg}': realigning the {which} VCF failed: {e}")
            per.append(cols)
            n_cl += info.n_clusters; n_in += len(s["pos"]); n_out += len(cols["pos"])
            kept["edge"] += info.n_edge; kept["limit"] += info.n_limit; kept["error"] += info.n_error
        out.append(per)
    print(f"[vcfdist_amd] realigned {which} VCF: {n_cl} clusters, {n_in} -> {n_out} hap-variants", file=sys.stderr)
    n_kept = sum(kept.values())
    if n_kept:
        print(f"[WARN  vcfdist_amd] {which} VCF: {n_kept} cluster(s) NOT REALIGNED, their variants kept as read: {kept['edge']} starting at "
              f"the contig's first base, {kept['limit']} beyond the memory limit of one alignment, {kept['error']} with inconsistent variants",
              file=sys.stderr)
        if args.strict:
            raise SystemExit(f"ERROR: {which} VCF: {n_kept} cluster(s) not realigned (--strict)")
    return dict(cs, vars=out)


def integer(lo, hi, invalid, outside):
    """an option's integer within lo..hi (hi None: unbounded), read with the messages given; `invalid` is formatted with the text"""
    def parse(v):
        try:
            x = int(v)
        except ValueError:
            raise argparse.ArgumentTypeError(invalid.format(v))
        if x < lo or (hi is not None and x > hi):
            raise argparse.ArgumentTypeError(outside)
        return x
    return parse


def eval_penalty(what):
    """an evaluation penalty as globals.cpp:274-335 reads it: an integer, non-negative"""
    return integer(0, None, f"Invalid {what} provided", f"Must provide non-negative {what}")


bootstrap_replicates = integer(1, A.BOOT_MAX_REPLICATES, "Invalid number of bootstrap replicates '{}'",
                               f"Must provide 1 to {A.BOOT_MAX_REPLICATES} bootstrap replicates")
bootstrap_seed = integer(0, 2 ** 64 - 1, "Invalid bootstrap seed '{}'", "Must provide a bootstrap seed of 0 to 2^64 - 1")
error_window = integer(0, 2 ** 31 - 1, "Invalid error window '{}'", "Must provide an error window of 0 to 2147483647 bases")


def argument_parser():
    ap = argparse.ArgumentParser(prog="python -m vcfdist_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("query"); ap.add_argument("truth"); ap.add_argument("fasta")
    ap.add_argument("-b", "--bed")
    ap.add_argument("-f", "--filter", default="", help="comma-separated FILTER ids to keep")
    ap.add_argument("-l", "--largest-variant", type=int, default=5000, dest="max_size")
    ap.add_argument("-mn", "--min-qual", type=int, default=0)
    ap.add_argument("-mx", "--max-qual", type=int, default=60)
    ap.add_argument("-c", "--cluster", nargs="+", default=["biwfa"], help="biwfa | gap N | size N")
    ap.add_argument("-i", "--max-iterations", type=int, default=4)
    ap.add_argument("-s", "--max-supercluster-size", type=int, default=10000)
    ap.add_argument("-x", "--mismatch-penalty", type=int, default=5, dest="sub")
    ap.add_argument("-o", "--gap-open-penalty", type=int, default=6, dest="open")
    ap.add_argument("-e", "--gap-extend-penalty", type=int, default=2, dest="extend")
    ap.add_argument("-ct", "--credit-threshold", type=float, default=0.7)
    ap.add_argument("-pt", "--phasing-threshold", type=float, default=0.6, dest="phase_threshold")
    ap.add_argument("-sv", "--sv-threshold", type=int, default=50)
    ap.add_argument("--reach-min-gap", type=int, default=10)
    ap.add_argument("-p", "--prefix", default="./", help="prefix of the output files")
    ap.add_argument("-n", "--no-output-files", action="store_true")
    ap.add_argument("--strict", action="store_true",
                    help="end with an error when a supercluster exceeds an implementation limit of the GPU path (more than eight swap "
                         "sources on one position, an alignment the dense kernels cannot place) instead of warning and leaving its "
                         "variants out of the counts and tables")
    ap.add_argument("--device", type=int, default=None, help="HIP device (default: LOCAL_RANK, else 0)")
    ap.add_argument("-d", "--distance", action="store_true", help="alignment-distance metrics (distance.tsv, distance-summary.tsv, edits.tsv)")
    ap.add_argument("-ex", "--eval-mismatch-penalty", type=eval_penalty("evaluation mismatch penalty"), default=3, dest="eval_sub")
    ap.add_argument("-eo", "--eval-gap-open-penalty", type=eval_penalty("eval gap-opening penalty"), default=2, dest="eval_open")
    ap.add_argument("-ee", "--eval-gap-extend-penalty", type=eval_penalty("eval gap-extension penalty"), default=1, dest="eval_extend")
    ap.add_argument("-rq", "--realign-query", action="store_true", help="realign the query variants before the evaluation")
    ap.add_argument("-rt", "--realign-truth", action="store_true", help="realign the truth variants before the evaluation")
    ap.add_argument("-ro", "--realign-only", action="store_true", help="stop after the realignment (query.vcf / truth.vcf)")
    ap.add_argument("--stratify", metavar="FILE",
                    help="strata list (one name<TAB>path of a BED per line, paths relative to the list): the counters of the one "
                         "evaluation are also cut by region (stratified-precision-recall.tsv, stratified-precision-recall-summary.tsv)")
    ap.add_argument("--stratify-repeats", action="store_true",
                    help="the default repeat strata (bases covered by a 16-, 24- or 32-mer that occurs more than once in the FASTA, on "
                         "either strand), built on the GPU, behind those of --stratify or alone; their intervals are written to "
                         "repeat-strata.bed")
    ap.add_argument("--stratify-long-repeats", action="store_true",
                    help="the default long repeat strata (bases covered by a 64-, 100- or 250-mer that occurs more than once in the FASTA, on "
                         "either strand), built on the GPU in one more genome-wide pass, behind the strata of --stratify and "
                         "--stratify-repeats; also writes long-repeat-strata.bed")
    ap.add_argument(NEAR_OPTION, metavar="K:M[,K:M...]",
                    help="near-repeat strata (bases covered by a K-mer that occurs again in the FASTA, on either strand, with at most M "
                         "substitutions; M 0 to 3, K 8 (M + 1) to 32, up to 4 entries), built on the GPU in one more genome-wide pass, "
                         "named near_k<K>_m<M>, behind the strata of --stratify-long-repeats; also writes near-repeat-strata.bed")
    ap.add_argument("--stratify-context", action="store_true",
                    help="the default sequence-context strata (homopolymers, short tandem repeats, GC bands), built on the GPU from the "
                         "FASTA, behind those of --stratify or alone; their intervals are written to context-strata.bed")
    ap.add_argument("--stratify-variants", action="store_true",
                    help="the default variant strata (transitions / transversions, indel size bins, hom / het, isolated / crowded), made "
                         "on the GPU from the variant tables, behind those of --stratify and --stratify-context or alone; "
                         "variant-strata.tsv lists them with their numbers of members")
    ap.add_argument("--stratify-derive", metavar="NAME=EXPR", action="append", default=[],
                    help="a stratum derived on the GPU from the membership bits of the strata in front of it (repeatable): operands are "
                         "stratum names, or globs with '*' that stand for the union of what they match; operators | & ! and parentheses; "
                         "!x is every hap-variant that is not a member of x.  Needs another --stratify* option; the derived strata follow "
                         "every other stratum in command-line order and are listed in derived-strata.tsv")
    ap.add_argument("--stratify-cross", metavar="LIST:LIST", action="append", default=[],
                    help="the strata a&b of every pair of two lists of globs (glob[,glob...]; repeatable), behind the derived strata, which "
                         "the lists may name; at most 512 derived plus crossed strata in all")
    ap.add_argument("--bootstrap", metavar="N", type=bootstrap_replicates, default=0,
                    help="resample the counters N times (1 to 100000) over superclusters on the GPU: 95 %% percentile intervals for "
                         "precision, recall and F1 (bootstrap-precision-recall-summary.tsv, bootstrap-replicates.tsv)")
    ap.add_argument("--bootstrap-seed", metavar="S", type=bootstrap_seed, default=1, help="seed of the bootstrap weights (default 1)")
    ap.add_argument("--classify-errors", action="store_true",
                    help="why each query FP and truth FN is wrong (right allele with the wrong genotype / on the aligned / on the other "
                         "haplotype, another allele at the site, something near, nothing), classified on the GPU: error-classes.tsv, "
                         "error-classes-summary.tsv")
    ap.add_argument("--error-window", metavar="N", type=error_window, default=None,
                    help="bases within which a variant of the other callset counts as near (default 50; needs --classify-errors)")
    ap.add_argument("--classify-matches", action="store_true",
                    help="how each TP was matched (exact: an allele-for-allele comparison finds it; shifted; regrouped; partial), "
                         "from the sync groups on the GPU: match-kinds.tsv, match-kinds-summary.tsv")
    ap.add_argument("--cut-classes", action="store_true",
                    help="cut the error classes / match kinds by the strata and resample them as well (needs --classify-errors or "
                         "--classify-matches, and a --stratify* option or --bootstrap): stratified-error-classes.tsv, "
                         "stratified-error-classes-summary.tsv, bootstrap-error-classes-summary.tsv and the match-kinds counterparts")
    ap.add_argument("--shard", default="superclusters", choices=["superclusters", "contigs"],
                    help="several ranks (torch.distributed.run, one per GPU): deal every contig's superclusters over the ranks "
                         "(default; balanced whatever the contigs' sizes) or whole contigs")
    return ap


def parse(argv=None):
    """the arguments, checked against each other: every error an option can be without a file having been opened"""
    args = argument_parser().parse_args(argv)
    args.cluster_gap = 50
    if args.cluster[0] in ("gap", "size") and len(args.cluster) > 1:
        args.cluster_gap = int(args.cluster[1])
    args.cluster = args.cluster[0]
    args.near = near_strata(args.stratify_near_repeats) if args.stratify_near_repeats is not None else []
    if args.max_size + 2 > args.max_supercluster_size:          # globals.cpp:478-481
        raise SystemExit("ERROR: Max supercluster size (-s) must be at least two larger than max variant size (-l).")
    if args.error_window is not None and not args.classify_errors:
        raise SystemExit("ERROR: --error-window needs --classify-errors")
    if args.cut_classes and not (args.classify_errors or args.classify_matches):
        raise SystemExit("ERROR: --cut-classes needs --classify-errors or --classify-matches")
    if args.cut_classes and not (stratifying(args) or args.bootstrap):
        raise SystemExit("ERROR: --cut-classes needs --stratify, --stratify-context, --stratify-variants or --bootstrap")
    if (args.realign_query or args.realign_truth) and (args.sub < 1 or args.extend < 1):
        raise SystemExit("ERROR: realignment needs a mismatch penalty (-x) and a gap-extension penalty (-e) of at least 1")
    return args


def setup_ranks(args):
    """one process per GPU under torch.distributed.run: every contig's superclusters are dealt over the ranks (--shard; the
    per-supercluster phasing is all-gathered, a contig's phasing needs all of it), the counters are summed with one all-reduce
    (RCCL), the result records are gathered, and rank 0 writes the files.  Selects this process's GPU and brings the group up."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if args.distance and world > 1:
        raise SystemExit("ERROR: -d/--distance runs on one rank only (its edit records are not gathered over ranks): "
                         "run it without torch.distributed.run")
    if (args.realign_query or args.realign_truth) and world > 1:
        raise SystemExit("ERROR: -rq/-rt realignment runs on one rank only (the realigned callsets are not sharded): "
                         "run it without torch.distributed.run")
    device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    one_gpu = bool(os.environ.get("VCFDIST_ONE_GPU"))      # plumbing check on a one-GPU box: every rank uses device 0, gloo
    if one_gpu and args.device is None:
        device = 0
    try:      # this process's GPU, before anything allocates page-locked staging memory (it would otherwise initialise device 0)
        api.lib().vpr_select_device(int(device))
    except api.VprError:
        pass
    ranks = Ranks(rank, world, device)
    if world > 1:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "nccl" if not one_gpu and torch.cuda.is_available() and torch.cuda.device_count() > device else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(device)
        dist.init_process_group(backend=backend)
        ranks.dist, ranks.cdev, ranks.by_sc = dist, None if backend == "gloo" else f"cuda:{device}", args.shard == "superclusters"
    return ranks


def plan_strata(args):
    """--stratify*: the strata list and every BED it names, read and checked before any input is opened, and behind the list's strata
    the defaults of every family that is on.  -> StrataPlan, or None without such an option"""
    if not stratifying(args):
        for option in (DERIVE_OPTION, CROSS_OPTION):
            if option_on(args, option):
                raise SystemExit(f"ERROR: {option} needs another --stratify* option")
        return None
    plan = StrataPlan()
    if args.stratify:
        try:
            names, plan.beds = IO.read_strata(args.stratify)
        except IOError as e:
            raise SystemExit(f"ERROR: {e}")
        plan.names = list(names)
    for fam in plan.ordered:
        if fam is plan.near:
            if not args.near:
                continue
            fam.names, fam.specs = [api.nearrepeat_name(sp) for sp in args.near], args.near
        elif not option_on(args, fam.option):
            continue
        else:
            fam.names, fam.specs = fam.defaults()
        for n in fam.names:
            if n in plan.names:
                raise SystemExit(f"ERROR: strata list '{args.stratify}': duplicate stratum name '{n}' (a {fam.word} stratum of {fam.option})")
        plan.names += fam.names
    derive_strata(args, plan)
    return plan


DERIVE_OPTION, CROSS_OPTION = "--stratify-derive", "--stratify-cross"


def derive_strata(args, plan):
    """--stratify-derive, --stratify-cross: every entry compiled by the library (one compiler for both command lines: its messages)
    against the names in front of it -- the derived entries in command-line order, then the crossed pairs, option by option"""
    dv = plan.derived

    def add(option, name, kind, expression, code):
        if len(dv.names) == A.DV_MAX_CLI:
            raise SystemExit(f"ERROR: {option}: more than {A.DV_MAX_CLI} derived and crossed strata")
        dv.add(name, kind, expression, code)
        plan.names.append(name)
    try:
        for entry in args.stratify_derive:
            option = DERIVE_OPTION
            name, code = api.derive_compile(entry, plan.names)
            add(option, name, A.DV_KIND_DERIVE, entry.split("=", 1)[1], code)
        for entry in args.stratify_cross:
            option = CROSS_OPTION
            for a, b in api.derive_cross(entry, plan.names):
                name = plan.names[a] + "&" + plan.names[b]
                add(option, name, A.DV_KIND_CROSS, name, (a, b, A.DV_AND))
    except api.VprError as e:
        raise SystemExit(f"ERROR: {option}: {e}")


EMPTY_SLOT = dict(pos=np.zeros(0, np.int32), rlen=np.zeros(0, np.int32), type=np.zeros(0, np.uint8), var_qual=np.zeros(0, np.float32),
                  phase_set=np.zeros(0, np.int32), ref_len=np.zeros(0, np.int32), alt_len=np.zeros(0, np.int32),
                  ref_off=np.zeros(0, np.int64), alt_off=np.zeros(0, np.int64), pool=np.zeros(1, np.uint8))


@dataclass
class Inputs:
    """what the run reads (Inputs in main.cpp): the callsets inside the -b BED, the FASTA, the contigs to evaluate in the reference's
    order, and the command line as the files record it"""
    q: dict; t: dict; fasta: dict; bed: object; contigs: list; cmd: str

    def slots_of(self, ctg):
        qs = self.q["vars"][self.q["contigs"].index(ctg)] if ctg in self.q["contigs"] else [EMPTY_SLOT, EMPTY_SLOT]
        ts = self.t["vars"][self.t["contigs"].index(ctg)] if ctg in self.t["contigs"] else [EMPTY_SLOT, EMPTY_SLOT]
        return [qs[0], qs[1], ts[0], ts[1]]

    def header_of(self, ctg):
        """a contig's length and ploidy (superclusterData ctor, cluster.cpp:134-157): the query's header wins, then the truth's"""
        src = self.q if ctg in self.q["contigs"] else self.t
        if ctg in src["contigs"]:
            j = src["contigs"].index(ctg)
            return src["lengths"][j], src["ploidy"][j]
        return len(self.fasta[ctg]), 0      # a BED contig neither callset lists (check_contigs appends it, ploidy 0)


def read_inputs(args, argv):
    """both callsets, the FASTA, with -rq / -rt the callsets as read (orig-query.vcf, orig-truth.vcf, main.cpp:50-180), and the contigs"""
    filters = tuple(f for f in args.filter.split(",") if f)
    bed = IO.Bed(args.bed) if args.bed else None
    kw = dict(min_qual=args.min_qual, max_qual=args.max_qual, max_size=args.max_size, cluster_min_gap=args.cluster_gap, filters=filters)
    q = IO.read_vcf(args.query, bed, **kw)
    t = IO.read_vcf(args.truth, bed, **kw)
    fasta = IO.read_fasta(args.fasta)
    if not args.no_output_files and args.realign_query:
        RP.write_vcf(args.prefix + "orig-query.vcf", q, fasta)
    if not args.no_output_files and args.realign_truth:
        RP.write_vcf(args.prefix + "orig-truth.vcf", t, fasta)
    contigs = check_contigs(q, t, fasta, bed)
    return Inputs(q, t, fasta, bed, contigs, " ".join(["vcfdist"] + list(sys.argv[1:] if argv is None else argv)))


def realign_inputs(inp, args, device):
    """-rq / -rt: each callset realigned in place of its columns.  -> True when -ro ends the run here, behind the realigned VCFs
    and the parameters (written first by the reference, main.cpp:35)"""
    write = not args.no_output_files
    if args.realign_query:
        inp.q = realign_callset("query", inp.q, inp.fasta, args, device=device)
        if args.realign_only and write:
            RP.write_vcf(args.prefix + "query.vcf", inp.q, inp.fasta)
    if args.realign_truth:
        inp.t = realign_callset("truth", inp.t, inp.fasta, args, device=device)
    if args.realign_only:
        if args.realign_truth and write:
            RP.write_vcf(args.prefix + "truth.vcf", inp.t, inp.fasta)
        if write:
            RP.write_parameters(args.prefix, args, inp.cmd)
    return args.realign_only


def evaluate_contigs(inp, args, ranks, plan, tot):
    """the contig loop: all of this rank's contigs prepared, then evaluated, their counts added to tot.  By superclusters every rank
    clusters and marshals every contig (host work and the biWFA clustering, done redundantly) and evaluates its share of each; by
    contigs a rank does everything for the contigs dealt to it.  -> what the writers need per contig ordinal, and -d's edit sets"""
    from . import shard
    contigs, fasta = inp.contigs, inp.fasta
    weights = [sum(len(s["pos"]) for s in inp.slots_of(c)) + 1 for c in contigs]
    mine = list(range(len(contigs))) if ranks.by_sc else shard.deal_contigs(weights, ranks.world)[ranks.rank]
    # everything in front of the path for all of this rank's contigs first: input the library refuses ends the run here,
    # like the reference's ERROR(), before anything has been evaluated or written
    prepared = {}
    for k in mine:
        try:
            prepared[k] = prepare_contig(contigs[k], fasta[contigs[k]], inp.slots_of(contigs[k]), args, device=ranks.device)
        except api.VprError as e:
            raise SystemExit(f"ERROR: contig '{contigs[k]}': {e}")
    reports = {}
    dist_sets = [] if args.distance else None
    for k in mine:
        ctg = contigs[k]
        try:      # the library's explicit refusals end the run like the reference's ERROR()
            counts, tables = evaluate_contig(prepared.pop(k), args, ranks, plan, tot, dist_sets=dist_sets, ordinal=k)
            tot.total += counts
            if plan is not None and plan.ctx.specs and ctg not in plan.ctx.rows and (ranks.rank == 0 or not ranks.by_sc):
                context_only(ctg, fasta[ctg], plan.ctx, args, device=ranks.device)
        except api.VprError as e:
            raise SystemExit(f"ERROR: contig '{ctg}': {e}")
        if not args.no_output_files:
            reports[k] = (ctg, *inp.header_of(ctg), inp.slots_of(ctg), tables)
    return reports, dist_sets


def reduce_ranks(args, ranks, plan, tot, reports):
    """the one all-reduce: every array of tot.tally summed over the ranks.  By contigs the ranks also exchange what only the
    contig's rank has: the writers' tables, the context intervals, and the device times (summed).  -> the reports of all contigs"""
    from . import shard
    dist = ranks.dist
    if dist is None:
        return reports
    unpack(tot.tally, shard.allreduce_tally(pack(tot.tally), device=ranks.cdev))
    if ranks.by_sc:         # (by superclusters every rank already holds every contig's gathered tables)
        return reports
    gathered = [None] * ranks.world
    dist.all_gather_object(gathered, reports)
    reports = {k: v for part in gathered for k, v in part.items()}
    if plan is not None and plan.ctx.specs:
        dist.all_gather_object(gathered, plan.ctx.rows)
        plan.ctx.rows = {k: v for part in gathered for k, v in part.items()}
    # the device times that are summed over the ranks, as (owner, attribute): one list, gathered once
    times = [(fam, "ms") for fam in ((plan.ctx, plan.vs) if plan is not None else ()) if fam.specs]
    times += [(plan.derived, "ms")] if plan is not None and plan.derived.names else []
    times += [(p, "ms") for p in tot.passes] + [(p, "cut_ms") for p in tot.passes if args.cut_classes]
    dist.all_gather_object(gathered, tuple(getattr(owner, name) for owner, name in times))
    for i, (owner, name) in enumerate(times):
        setattr(owner, name, sum(part[i] for part in gathered))
    return reports


def write_outputs(args, inp, plan, tot, reports):
    """every file of the evaluation (rank 0); the writers are looked up in report when they are called"""
    mn, mx, prefix = args.min_qual, args.max_qual, args.prefix
    RP.write_precision_recall(prefix, tot.total, mn, mx)
    RP.write_parameters(prefix, args, inp.cmd)
    if plan is not None:
        RP.write_stratified(prefix, plan.names, tot.strat, mn, mx)
        for fam in plan.kmer:
            getattr(RP, fam.write)(prefix, inp.contigs, fam.names, fam.rows)
        if plan.ctx.specs:
            RP.write_context_bed(prefix, inp.contigs, plan.ctx.names, plan.ctx.rows)
        if plan.vs.specs:
            RP.write_variant_strata(prefix, plan.vs.names, plan.vs.specs, tot.vs_members[0], tot.vs_members[1])
        if plan.derived.names:
            dv = plan.derived
            RP.write_derived_strata(prefix, dv.names, dv.kinds, dv.expressions, tot.dv_members[0], tot.dv_members[1])
    for p in tot.passes:
        getattr(RP, p.write)(prefix, p.counts, tot.total, mn, mx)
    if tot.boot is not None:
        RP.write_bootstrap(prefix, tot.total, tot.boot, args.bootstrap_seed, mn, mx)
        if plan is not None:
            RP.write_bootstrap_stratified(prefix, plan.names, tot.strat, tot.boot_strat, args.bootstrap_seed, mn, mx)
    for p in tot.passes:
        if p.strata is not None:
            getattr(RP, p.write_strata)(prefix, plan.names, p.strata, tot.strat, mn, mx)
        if p.boot is not None:
            getattr(RP, p.write_boot)(prefix, p.counts, tot.total, p.boot, mn, mx)
    ctgs = [RP.Contig(c, ln, pl, inp.fasta[c], sl, *tb) for c, ln, pl, sl, tb in (reports[k] for k in sorted(reports))]
    RP.write_results(prefix, ctgs, cmd=inp.cmd, credit_threshold=args.credit_threshold)
    if args.realign_query:
        RP.write_vcf(prefix + "query.vcf", inp.q, inp.fasta)
    if args.realign_truth:
        RP.write_vcf(prefix + "truth.vcf", inp.t, inp.fasta)


def report(args, plan, tot, rows):
    """rank 0's closing lines on stderr, one per option, then the PRECISION-RECALL SUMMARY on stdout"""
    say = lambda line: print("[vcfdist_amd] " + line, file=sys.stderr)
    if plan is not None:
        say(f"stratified: {len(plan.names)} strata, {int(tot.seen_none[1])} of {int(tot.seen_none[0])} hap-variants in none of them")
        for fam in plan.kmer:
            n_iv = sum(len(a) for per in fam.rows.values() for a, _ in per)
            if fam is plan.near:
                starts = ", ".join(f"{int(v)} valid and {int(r)} near-repeated starts (k={sp.k}, m={sp.m})" for sp, v, r in zip(fam.specs, *fam.stats[:2]))
                starts += f", {int(fam.stats[2].sum())} compares, longest run {int(fam.stats[3].max())}"
            else:
                starts = ", ".join(f"{int(v)} valid and {int(r)} repeated starts (k={sp.k})" for sp, v, r in zip(fam.specs, *fam.stats))
            say(f"{fam.word} strata: {n_iv} intervals of {len(fam.specs)} strata, {starts}, {fam.ms:.3f} ms on the device")
        if plan.ctx.specs:
            n_iv = sum(len(a) for per in plan.ctx.rows.values() for a, _ in per)
            say(f"context strata: {n_iv} intervals of {len(plan.ctx.specs)} strata, {plan.ctx.ms:.3f} ms on the device")
        if plan.vs.specs:
            say(f"variant strata: {len(plan.vs.specs)} strata, {plan.vs.ms:.3f} ms on the device")
        if plan.derived.names:
            n_cross = sum(k == A.DV_KIND_CROSS for k in plan.derived.kinds)
            say(f"derived strata: {len(plan.derived.names)} strata ({len(plan.derived.names) - n_cross} derived, {n_cross} crossed), "
                f"{plan.derived.ms:.3f} ms on the device")
    for p in tot.passes:
        print(p.line(p), file=sys.stderr)
    if args.cut_classes:
        what = ([f"{len(plan.names)} strata"] if plan is not None else []) + ([f"{args.bootstrap} replicates"] if args.bootstrap else [])
        for p in tot.passes:
            say(f"{p.noun} cut: {', '.join(what)}, {p.cut_ms:.3f} ms on the device")
    if args.bootstrap:
        say(f"bootstrap: {args.bootstrap} replicates, seed {args.bootstrap_seed}, {tot.boot_ms:.3f} ms on the device")
    print("PRECISION-RECALL SUMMARY\n")
    print("TYPE\tTHRESHOLD\tTRUTH_TP\tQUERY_TP\tTRUTH_FN\tQUERY_FP\tPREC\t\tRECALL\t\tF1_SCORE\tF1_QSCORE")
    for r in rows:
        print("%s\t%s Q >= %-2d\t%-16d%-16d%-16d%-16d%f\t%f\t%f\t%f" % (S.NAMES[r.vartype], "BEST" if r.best else "NONE", r.qual,
              r.truth_tp, r.query_tp, r.truth_fn, r.query_fp, r.precision, r.recall, r.f1_score, r.f1_qscore))
        if r.best:
            print()


def main(argv=None):
    """the stages, in the order and under the names of main.cpp's -> the summary's rows ([] under -ro)"""
    args = parse(argv)
    ranks = setup_ranks(args)
    plan = plan_strata(args)        # (before any input is opened)
    inp = read_inputs(args, argv)
    if realign_inputs(inp, args, ranks.device):
        return []
    try:        # the genome-wide k-mer passes, before the contig loop
        for fam in plan.kmer if plan is not None else ():
            kmer_strata(fam, inp.fasta, args, device=ranks.device)
    except api.VprError as e:
        raise SystemExit(f"ERROR: {e}")
    tot = Totals(args, plan)
    reports, dist_sets = evaluate_contigs(inp, args, ranks, plan, tot)
    reports = reduce_ranks(args, ranks, plan, tot, reports)
    rows = S.pr_summary(tot.total, args.min_qual, args.max_qual)
    if dist_sets is not None:       # write_distance (printed even with -n) and write_edits, edit.cpp:134-280
        text = RP.write_distance(args.prefix, dist_sets, args.min_qual, args.max_qual, args.eval_sub, args.eval_open, args.eval_extend,
                                 verbosity=1, write_files=not args.no_output_files)
        if not args.no_output_files:
            RP.write_edits(args.prefix + "edits.tsv", dist_sets)
        print(text)
    if ranks.rank == 0:
        if not args.no_output_files:
            write_outputs(args, inp, plan, tot, reports)
        report(args, plan, tot, rows)
    if ranks.dist is not None:
        ranks.dist.barrier()
        ranks.dist.destroy_process_group()
    return rows


if __name__ == "__main__":
    main()
