"""ctypes mirror of include/vcfdist_report.h: the TSV tables and the summary VCF behind the path."""
import ctypes as C

import numpy as np

from . import _abi as A
from . import api

P_f32 = C.POINTER(C.c_float)


class VrpHap(C.Structure):
    _fields_ = [("n_var", C.c_int32), ("pos", A.P_i32), ("type", A.P_u8), ("loc", A.P_u8), ("var_qual", P_f32),
                ("phase_set", A.P_i32), ("ref_len", A.P_i32), ("alt_len", A.P_i32), ("ref_off", A.P_i64), ("alt_off", A.P_i64),
                ("pool", A.P_u8), ("n_cluster", C.c_int32), ("cluster_beg", A.P_i32),
                ("errtype", A.P_u8 * 2), ("credit", P_f32 * 2), ("sync_group", A.P_i32 * 2), ("ref_ed", A.P_i32 * 2),
                ("query_ed", A.P_i32 * 2)]


class VrpContig(C.Structure):
    _fields_ = [("name", C.c_char_p), ("length", C.c_int32), ("ploidy", C.c_int32), ("seq", A.P_u8), ("seq_len", C.c_int64),
                ("hap", VrpHap * 4), ("n_sc", C.c_int32), ("sc_beg", A.P_i32), ("sc_end", A.P_i32), ("sc_brk", A.P_i32 * 4),
                ("sc_phase", A.P_i32), ("pb_phase", A.P_i32), ("orig_phase_dist", A.P_i32), ("swap_phase_dist", A.P_i32),
                ("sc_phase_set", A.P_i32), ("n_pb", C.c_int32), ("phase_block", A.P_i32), ("n_switches", C.c_int32),
                ("n_flips", C.c_int32), ("switches", A.P_i32), ("flips", A.P_i32)]


EXPORTED = ["vrp_phase_blocks", "vrp_write_precision_recall", "vrp_write_stratified", "vrp_write_context_bed", "vrp_write_repeat_bed", "vrp_write_long_repeat_bed", "vrp_write_near_repeat_bed", "vrp_write_derived_strata", "vrp_write_bootstrap", "vrp_write_bootstrap_stratified", "vrp_write_phase_blocks", "vrp_write_superclusters",
            "vrp_write_switchflips", "vrp_write_phasing_summary", "vrp_ng50",
            "vrp_write_variants", "vrp_write_summary_vcf", "vrp_write_distance", "vrp_write_edits", "vrp_write_vcf", "vrp_last_error"]


class ReportError(RuntimeError):
    pass


def _check(rc, what):
    if rc:
        L = api.lib()
        L.vrp_last_error.restype = C.c_char_p
        raise ReportError(f"{what} failed ({rc}): {L.vrp_last_error().decode()}")


def phase_blocks(sc_phase_set):
    """first supercluster of each phase block + n_sc (phaseblockData ctor, phase.cpp:229-262)"""
    ps = np.ascontiguousarray(sc_phase_set, np.int32)
    out = np.zeros(len(ps) + 1, np.int32)
    L = api.lib()
    L.vrp_phase_blocks.argtypes = [A.P_i32, C.c_int32, A.P_i32]
    n = L.vrp_phase_blocks(A._ptr(ps, C.c_int32), len(ps), A._ptr(out, C.c_int32))
    if n < 0:
        raise ReportError(f"vrp_phase_blocks failed ({n})")
    return out[:n + 1].copy()


_C32 = ("pos", "phase_set", "ref_len", "alt_len")


class Contig:
    """Everything the writers need of one contig.  slots: the four column dicts of vcfdist_amd.io (Q1, Q2, T1, T2);
    clusters: the four cluster tables after superclustering (Superclusters.clusters); sc: Superclusters; res: the
    Results of the path (or any object with the same per-variant arrays); pb / switches / flips: summary.phase()."""

    def __init__(self, name, length, ploidy, seq, slots, clusters, sc, res, sc_phase_set, pb_phase, switches, flips):
        self.keep = []
        k = self._own
        c = VrpContig()
        self.name = name.encode()
        c.name = self.name
        c.length, c.ploidy = int(length), int(ploidy)
        seq = np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, np.uint8)
        c.seq, c.seq_len = A._ptr(k(seq, np.uint8), C.c_uint8), len(seq)
        for i, s in enumerate(slots):
            h = c.hap[i]
            n = len(s["pos"])
            h.n_var = n
            for f in _C32:
                setattr(h, f, A._ptr(k(s[f], np.int32), C.c_int32))
            h.type = A._ptr(k(s["type"], np.uint8), C.c_uint8)
            h.var_qual = A._ptr(k(s["var_qual"], np.float32), C.c_float)
            h.ref_off = A._ptr(k(s["ref_off"], np.int64), C.c_int64)
            h.alt_off = A._ptr(k(s["alt_off"], np.int64), C.c_int64)
            h.pool = A._ptr(k(s["pool"] if len(s["pool"]) else np.zeros(1, np.uint8), np.uint8), C.c_uint8)
            cl = clusters[i]
            h.n_cluster = cl.n
            if cl.n:
                h.cluster_beg = A._ptr(k(cl.var_beg, np.int32), C.c_int32)
            for w in range(2):
                h.errtype[w] = A._ptr(k(res.errtype[i][w], np.uint8), C.c_uint8)
                h.credit[w] = A._ptr(k(res.credit[i][w], np.float32), C.c_float)
                h.sync_group[w] = A._ptr(k(res.sync_group[i][w], np.int32), C.c_int32)
                h.ref_ed[w] = A._ptr(k(res.ref_ed[i][w], np.int32), C.c_int32)
                h.query_ed[w] = A._ptr(k(res.query_ed[i][w], np.int32), C.c_int32)
        c.n_sc = sc.n
        i32 = lambda a: A._ptr(k(a, np.int32), C.c_int32)
        c.sc_beg, c.sc_end = i32(sc.beg), i32(sc.end)
        for i in range(4):
            c.sc_brk[i] = i32(sc.brk[i])
        c.sc_phase, c.pb_phase = i32(res.sc_phase), i32(pb_phase)
        c.orig_phase_dist, c.swap_phase_dist = i32(res.orig_phase_dist), i32(res.swap_phase_dist)
        c.sc_phase_set = i32(sc_phase_set)
        self.phase_block = phase_blocks(sc_phase_set)
        c.n_pb = len(self.phase_block) - 1
        c.phase_block = i32(self.phase_block)
        c.n_switches, c.n_flips = len(switches), len(flips)
        c.switches, c.flips = i32(switches), i32(flips)
        self.struct = c

    def _own(self, a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        self.keep.append(a)
        return a


def _array(contigs):
    arr = (VrpContig * max(len(contigs), 1))()
    for i, c in enumerate(contigs):
        arr[i] = c.struct
    return arr


def write_precision_recall(prefix, counts, min_qual, max_qual):
    cnt = np.ascontiguousarray(counts, np.int64)
    L = api.lib()
    L.vrp_write_precision_recall.argtypes = [C.c_char_p, A.P_i64, C.c_int32, C.c_int32]
    _check(L.vrp_write_precision_recall(prefix.encode(), A._ptr(cnt, C.c_int64), min_qual, max_qual), "vrp_write_precision_recall")


def write_stratified(prefix, names, counts, min_qual, max_qual):
    """stratified-precision-recall.tsv / -summary.tsv: counts int64 [n_strata][2][4][3][nq] (summary.pr_counts_strata)"""
    cnt = np.ascontiguousarray(counts, np.int64)
    if cnt.shape[0] != len(names):
        raise ReportError(f"{len(names)} stratum names for counts of {cnt.shape[0]} strata")
    L = api.lib()
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    L.vrp_write_stratified.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, A.P_i64, C.c_int32, C.c_int32]
    _check(L.vrp_write_stratified(prefix.encode(), arr, len(names), A._ptr(cnt, C.c_int64), min_qual, max_qual), "vrp_write_stratified")


def _write_strata_bed(entry, prefix, contigs, names, intervals):
    off, st, sp = [0], [], []
    for c in contigs:
        rows = intervals[c]
        if len(rows) != len(names):
            raise ReportError(f"contig '{c}': intervals of {len(rows)} strata for {len(names)} names")
        for a, b in rows:
            st.append(np.asarray(a, np.int32)); sp.append(np.asarray(b, np.int32))
            off.append(off[-1] + len(st[-1]))
    off = np.asarray(off, np.int64)
    st = np.ascontiguousarray(np.concatenate(st + [np.zeros(1, np.int32)]), np.int32)     # (never empty: a pointer is wanted)
    sp = np.ascontiguousarray(np.concatenate(sp + [np.zeros(1, np.int32)]), np.int32)
    f = getattr(api.lib(), entry)
    carr = (C.c_char_p * max(len(contigs), 1))(*[c.encode() for c in contigs])
    narr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    f.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_char_p), C.c_int32, A.P_i64, A.P_i32, A.P_i32]
    _check(f(prefix.encode(), carr, len(contigs), narr, len(names), A._ptr(off, C.c_int64), A._ptr(st, C.c_int32), A._ptr(sp, C.c_int32)), entry)


def write_context_bed(prefix, contigs, names, intervals):
    """context-strata.bed (include/vcfdist_context.h): contigs in evaluation order, names of the context strata in table order,
    intervals[contig] = [(starts, stops) per stratum]"""
    _write_strata_bed("vrp_write_context_bed", prefix, contigs, names, intervals)


def write_repeat_bed(prefix, contigs, names, intervals):
    """repeat-strata.bed (include/vcfdist_repeats.h): the same for the repeat strata, in the same format and order"""
    _write_strata_bed("vrp_write_repeat_bed", prefix, contigs, names, intervals)


def write_long_repeat_bed(prefix, contigs, names, intervals):
    """long-repeat-strata.bed (include/vcfdist_longrepeats.h): the same for the long repeat strata"""
    _write_strata_bed("vrp_write_long_repeat_bed", prefix, contigs, names, intervals)


def write_near_repeat_bed(prefix, contigs, names, intervals):
    """near-repeat-strata.bed (include/vcfdist_nearrepeats.h): the same for the near-repeat strata"""
    _write_strata_bed("vrp_write_near_repeat_bed", prefix, contigs, names, intervals)


def write_variant_strata(prefix, names, spec, n_query, n_truth):
    """variant-strata.tsv (include/vcfdist_varstrata.h): one row per variant stratum -- name, kind, parameters, and the numbers of
    query and of truth hap-variants that are members"""
    if not len(names) == len(spec) == len(n_query) == len(n_truth):
        raise ReportError(f"{len(names)} names, {len(spec)} spec entries, {len(n_query)} / {len(n_truth)} member counts")
    nq, nt = np.ascontiguousarray(n_query, np.int64), np.ascontiguousarray(n_truth, np.int64)
    if nq.size == 0:
        nq = nt = np.zeros(1, np.int64)
    L = api.lib()
    narr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    sarr = (A.VprVariantStratum * max(len(spec), 1))(*spec)
    L.vrp_write_variant_strata.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(A.VprVariantStratum), C.c_int32, A.P_i64, A.P_i64]
    _check(L.vrp_write_variant_strata(prefix.encode(), narr, sarr, len(names), A._ptr(nq, C.c_int64), A._ptr(nt, C.c_int64)),
           "vrp_write_variant_strata")


def write_derived_strata(prefix, names, kinds, expressions, n_query, n_truth):
    """derived-strata.tsv (include/vcfdist_derive.h): one row per derived or crossed stratum -- name, kind (A.DV_KIND_*), the
    expression as given (a&b for a cross), and the numbers of query and of truth hap-variants that are members"""
    if not len(names) == len(kinds) == len(expressions) == len(n_query) == len(n_truth):
        raise ReportError(f"{len(names)} names, {len(kinds)} kinds, {len(expressions)} expressions, {len(n_query)} / {len(n_truth)} member counts")
    nq, nt, kd = np.ascontiguousarray(n_query, np.int64), np.ascontiguousarray(n_truth, np.int64), np.ascontiguousarray(kinds, np.int32)
    if nq.size == 0:
        nq = nt = np.zeros(1, np.int64)
        kd = np.zeros(1, np.int32)
    L = api.lib()
    narr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    earr = (C.c_char_p * max(len(names), 1))(*[e.encode() for e in expressions])
    L.vrp_write_derived_strata.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), A.P_i32, C.POINTER(C.c_char_p), C.c_int32, A.P_i64, A.P_i64]
    _check(L.vrp_write_derived_strata(prefix.encode(), narr, A._ptr(kd, C.c_int32), earr, len(names), A._ptr(nq, C.c_int64), A._ptr(nt, C.c_int64)),
           "vrp_write_derived_strata")


def _write_label_counts(entry, prefix, label_counts, n_labels, counts, min_qual, max_qual):
    """the two files of a label pass (vrp_<entry>): label_counts int64 [2][4][n_labels][nq] beside counts int64 [2][4][3][nq]"""
    nq = max_qual - min_qual + 1
    lc, cnt = np.ascontiguousarray(label_counts, np.int64), np.ascontiguousarray(counts, np.int64)
    if lc.shape != (2, 4, n_labels, nq) or cnt.shape != (2, 4, 3, nq):
        raise ReportError(f"{entry}: counts of shapes {lc.shape} and {cnt.shape} for {nq} thresholds")
    fn = getattr(api.lib(), "vrp_" + entry)
    fn.argtypes = [C.c_char_p, A.P_i64, A.P_i64, C.c_int32, C.c_int32]
    _check(fn(prefix.encode(), A._ptr(lc, C.c_int64), A._ptr(cnt, C.c_int64), min_qual, max_qual), "vrp_" + entry)


def write_error_classes(prefix, class_counts, counts, min_qual, max_qual):
    """error-classes.tsv and error-classes-summary.tsv (include/vcfdist_errclass.h): class_counts int64 [2][4][7][nq]
    (PrecisionRecall.errclass), counts int64 [2][4][3][nq] (summary.pr_counts) of the same evaluation, for the BEST threshold"""
    _write_label_counts("write_error_classes", prefix, class_counts, A.EC_CLASSES, counts, min_qual, max_qual)


def write_match_kinds(prefix, kind_counts, counts, min_qual, max_qual):
    """match-kinds.tsv and match-kinds-summary.tsv (include/vcfdist_matchkind.h): kind_counts int64 [2][4][4][nq]
    (PrecisionRecall.matchkind), counts int64 [2][4][3][nq] (summary.pr_counts) of the same evaluation, for the BEST threshold"""
    _write_label_counts("write_match_kinds", prefix, kind_counts, A.MK_KINDS, counts, min_qual, max_qual)


def _write_label_stratified(entry, prefix, names, label_counts, n_labels, counts, min_qual, max_qual):
    """the two stratified files of a label pass (vrp_<entry>): label_counts int64 [n_strata][2][4][n_labels][nq] beside counts
    int64 [n_strata][2][4][3][nq] (summary.pr_counts_strata)"""
    nq, n = max_qual - min_qual + 1, len(names)
    lc, cnt = np.ascontiguousarray(label_counts, np.int64), np.ascontiguousarray(counts, np.int64)
    if lc.shape != (n, 2, 4, n_labels, nq) or cnt.shape != (n, 2, 4, 3, nq):
        raise ReportError(f"{entry}: {n} stratum names, counts of shapes {lc.shape} and {cnt.shape} for {nq} thresholds")
    fn = getattr(api.lib(), "vrp_" + entry)
    fn.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, A.P_i64, A.P_i64, C.c_int32, C.c_int32]
    arr = (C.c_char_p * max(n, 1))(*[x.encode() for x in names])
    if n == 0:
        lc = cnt = np.zeros(1, np.int64)
    _check(fn(prefix.encode(), arr, n, A._ptr(lc, C.c_int64), A._ptr(cnt, C.c_int64), min_qual, max_qual), "vrp_" + entry)


def _write_label_bootstrap(entry, prefix, label_counts, n_labels, counts, label_boot, min_qual, max_qual):
    """the bootstrap file of a label pass (vrp_<entry>): label_boot int64 [n_rep][2][4][n_labels][nq] beside the point counts"""
    nq = max_qual - min_qual + 1
    lc, cnt, boot = (np.ascontiguousarray(x, np.int64) for x in (label_counts, counts, label_boot))
    if lc.shape != (2, 4, n_labels, nq) or cnt.shape != (2, 4, 3, nq) or boot.ndim != 5 or boot.shape[0] < 1 or boot.shape[1:] != lc.shape:
        raise ReportError(f"{entry}: counts of shapes {lc.shape}, {cnt.shape} and {boot.shape} for {nq} thresholds")
    fn = getattr(api.lib(), "vrp_" + entry)
    fn.argtypes = [C.c_char_p, A.P_i64, A.P_i64, A.P_i64, C.c_int32, C.c_int32, C.c_int32]
    _check(fn(prefix.encode(), A._ptr(lc, C.c_int64), A._ptr(cnt, C.c_int64), A._ptr(boot, C.c_int64), boot.shape[0], min_qual, max_qual),
           "vrp_" + entry)


def write_error_classes_stratified(prefix, names, class_counts, counts, min_qual, max_qual):
    """stratified-error-classes.tsv and stratified-error-classes-summary.tsv: class_counts int64 [n_strata][2][4][7][nq]
    (PrecisionRecall.errclass_strata), counts int64 [n_strata][2][4][3][nq] (summary.pr_counts_strata), for BEST per stratum"""
    _write_label_stratified("write_error_classes_stratified", prefix, names, class_counts, A.EC_CLASSES, counts, min_qual, max_qual)


def write_match_kinds_stratified(prefix, names, kind_counts, counts, min_qual, max_qual):
    """stratified-match-kinds.tsv and stratified-match-kinds-summary.tsv: kind_counts int64 [n_strata][2][4][4][nq]
    (PrecisionRecall.matchkind_strata), counts int64 [n_strata][2][4][3][nq] (summary.pr_counts_strata)"""
    _write_label_stratified("write_match_kinds_stratified", prefix, names, kind_counts, A.MK_KINDS, counts, min_qual, max_qual)


def write_error_classes_bootstrap(prefix, class_counts, counts, class_boot, min_qual, max_qual):
    """bootstrap-error-classes-summary.tsv: the point counts of write_error_classes and class_boot int64 [n_rep][2][4][7][nq]
    (PrecisionRecall.errclass_boot); every count column is followed by its 95 % percentile bounds, integers"""
    _write_label_bootstrap("write_error_classes_bootstrap", prefix, class_counts, A.EC_CLASSES, counts, class_boot, min_qual, max_qual)


def write_match_kinds_bootstrap(prefix, kind_counts, counts, kind_boot, min_qual, max_qual):
    """bootstrap-match-kinds-summary.tsv: the point counts of write_match_kinds and kind_boot int64 [n_rep][2][4][4][nq]
    (PrecisionRecall.matchkind_boot)"""
    _write_label_bootstrap("write_match_kinds_bootstrap", prefix, kind_counts, A.MK_KINDS, counts, kind_boot, min_qual, max_qual)


def write_bootstrap(prefix, counts, counts_boot, seed, min_qual, max_qual):
    """bootstrap-precision-recall-summary.tsv and bootstrap-replicates.tsv (include/vcfdist_bootstrap.h): counts int64
    [2][4][3][nq] (summary.pr_counts), counts_boot int64 [n_rep][2][4][3][nq] (summary.pr_counts_boot)"""
    cnt, boot = np.ascontiguousarray(counts, np.int64), np.ascontiguousarray(counts_boot, np.int64)
    if boot.ndim != 5 or boot.shape[1:] != cnt.shape:
        raise ReportError(f"replicate counts of shape {boot.shape} for point counts of shape {cnt.shape}")
    L = api.lib()
    L.vrp_write_bootstrap.argtypes = [C.c_char_p, A.P_i64, A.P_i64, C.c_int32, C.c_uint64, C.c_int32, C.c_int32]
    _check(L.vrp_write_bootstrap(prefix.encode(), A._ptr(cnt, C.c_int64), A._ptr(boot, C.c_int64), boot.shape[0], int(seed), min_qual, max_qual),
           "vrp_write_bootstrap")


def write_bootstrap_stratified(prefix, names, counts, counts_boot, seed, min_qual, max_qual):
    """stratified-bootstrap-precision-recall-summary.tsv: counts int64 [n_strata][2][4][3][nq], counts_boot int64
    [n_strata][n_rep][2][4][3][nq]"""
    cnt, boot = np.ascontiguousarray(counts, np.int64), np.ascontiguousarray(counts_boot, np.int64)
    if cnt.shape[0] != len(names) or boot.ndim != 6 or boot.shape[0] != len(names) or boot.shape[2:] != cnt.shape[1:]:
        raise ReportError(f"{len(names)} stratum names for point counts of shape {cnt.shape} and replicate counts of shape {boot.shape}")
    L = api.lib()
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    L.vrp_write_bootstrap_stratified.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, A.P_i64, A.P_i64, C.c_int32, C.c_uint64,
                                                 C.c_int32, C.c_int32]
    _check(L.vrp_write_bootstrap_stratified(prefix.encode(), arr, len(names), A._ptr(cnt, C.c_int64), A._ptr(boot, C.c_int64), boot.shape[1],
                                            int(seed), min_qual, max_qual), "vrp_write_bootstrap_stratified")


def write_results(prefix, contigs, cmd="", file_date=None, credit_threshold=0.7):
    """phase-blocks.tsv, superclusters.tsv, query.tsv, truth.tsv (write_results, print.cpp:575-878), switchflips.tsv and
    phasing-summary.tsv (phase.cpp:406-528) and summary.vcf"""
    L = api.lib()
    arr, n = _array(contigs), len(contigs)
    P = C.POINTER(VrpContig)
    L.vrp_write_phase_blocks.argtypes = [C.c_char_p, P, C.c_int32]
    L.vrp_write_superclusters.argtypes = [C.c_char_p, P, C.c_int32]
    L.vrp_write_variants.argtypes = [C.c_char_p, P, C.c_int32, C.c_int32]
    L.vrp_write_summary_vcf.argtypes = [C.c_char_p, P, C.c_int32, C.c_char_p, C.c_char_p, C.c_float]
    L.vrp_write_switchflips.argtypes = [C.c_char_p, P, C.c_int32]
    L.vrp_write_phasing_summary.argtypes = [C.c_char_p, P, C.c_int32]
    _check(L.vrp_write_phase_blocks((prefix + "phase-blocks.tsv").encode(), arr, n), "vrp_write_phase_blocks")
    _check(L.vrp_write_switchflips((prefix + "switchflips.tsv").encode(), arr, n), "vrp_write_switchflips")
    _check(L.vrp_write_phasing_summary((prefix + "phasing-summary.tsv").encode(), arr, n), "vrp_write_phasing_summary")
    _check(L.vrp_write_superclusters((prefix + "superclusters.tsv").encode(), arr, n), "vrp_write_superclusters")
    _check(L.vrp_write_variants((prefix + "query.tsv").encode(), arr, n, 0), "vrp_write_variants")
    _check(L.vrp_write_variants((prefix + "truth.tsv").encode(), arr, n, 1), "vrp_write_variants")
    _check(L.vrp_write_summary_vcf((prefix + "summary.vcf").encode(), arr, n, cmd.encode(),
                                   file_date.encode() if file_date else None, credit_threshold), "vrp_write_summary_vcf")


class VrpEdits(C.Structure):
    _fields_ = [("ctg", C.c_char_p), ("n", C.c_int64), ("sc", A.P_i32), ("hap", A.P_u8), ("pos", A.P_i32), ("type", A.P_u8),
                ("len", A.P_i32), ("min_qual", A.P_i32), ("max_qual", A.P_i32)]


def _edit_sets(sets):
    """[(contig name, dict of edit_* columns as PrecisionRecall.distance returns them)] -> (ctypes array, arrays kept alive)"""
    keep, arr = [], (VrpEdits * max(len(sets), 1))()
    for k, (name, d) in enumerate(sets):
        e = arr[k]
        nm = name.encode()
        keep.append(nm)
        e.ctg, e.n = nm, len(d["edit_sc"])
        for f, col, ct, dt in (("sc", "edit_sc", C.c_int32, np.int32), ("hap", "edit_hap", C.c_uint8, np.uint8),
                               ("pos", "edit_pos", C.c_int32, np.int32), ("type", "edit_type", C.c_uint8, np.uint8),
                               ("len", "edit_len", C.c_int32, np.int32), ("min_qual", "edit_min_qual", C.c_int32, np.int32),
                               ("max_qual", "edit_max_qual", C.c_int32, np.int32)):
            a = np.ascontiguousarray(d[col], dt)
            if len(a) == 0:
                a = np.zeros(1, dt)
            keep.append(a)
            setattr(e, f, A._ptr(a, ct))
    return arr, keep


def write_distance(prefix, sets, min_qual, max_qual, eval_sub, eval_open, eval_extend, verbosity=1, write_files=True):
    """distance.tsv and distance-summary.tsv under prefix (write_files) and the ALIGNMENT DISTANCE SUMMARY text, which is returned
    (editData::write_distance, edit.cpp:137-250; vrp_write_distance)"""
    arr, keep = _edit_sets(sets)
    L = api.lib()
    L.vrp_write_distance.argtypes = [C.c_char_p, C.POINTER(VrpEdits), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
    buf = C.create_string_buffer(1 << 16)
    n = L.vrp_write_distance((prefix or "").encode(), arr, len(sets), min_qual, max_qual, eval_sub, eval_open, eval_extend, verbosity,
                             1 if write_files else 0, buf, len(buf))
    if n < 0:
        _check(n, "vrp_write_distance")
    return buf.value.decode()


def write_edits(path, sets):
    """edits.tsv (editData::write_edits, edit.cpp:256-270; vrp_write_edits)"""
    arr, keep = _edit_sets(sets)
    L = api.lib()
    L.vrp_write_edits.argtypes = [C.c_char_p, C.POINTER(VrpEdits), C.c_int32]
    _check(L.vrp_write_edits(path.encode(), arr, len(sets)), "vrp_write_edits")


def write_parameters(prefix, args, cmd):
    """parameters.txt (write_params, print.cpp:30-56): the run's settings, one `key = value` per line, in the reference's order and
    formats (strings quoted, booleans true / false, the two thresholds and max_ram with %f).  Keys of stages this implementation
    does not have keep the reference's defaults (globals.h:41-59); realignment, eval penalties and distance are the run's."""
    b2s = lambda b: "true" if b else "false"
    L = api.lib()
    L.vpr_version.restype = C.c_char_p
    text = (
        "program = '%s'\nversion = '%s'\nout_prefix = '%s'\ncommand = '%s'\nreference_fasta = '%s'\n"
        "query_vcf = '%s'\ntruth_vcf = '%s'\nbed_file = '%s'\nwrite_outputs = %s\nfilters = '%s'\n"
        "min_var_qual = %d\nmax_var_qual = %d\nmax_var_size = %d\nsv_threshold = %d\n"
        "phase_threshold = %f\ncredit_threshold = %f\nrealign_truth = %s\nrealign_query = %s\n"
        "realign_only = %s\ncluster_method = '%s'\ncluster_min_gap = %d\n"
        "reach_min_gap = %d\nmax_cluster_itrs = %d\nmax_threads = %d\nmax_ram = %f\n"
        "sub = %d\nopen = %d\nextend = %d\neval_sub = %d\neval_open = %d\neval_extend = %d\ndistance = %s" % (
            "vcfdist_amd", L.vpr_version().decode(), prefix, cmd, args.fasta, args.query, args.truth, args.bed or "",
            b2s(not args.no_output_files), args.filter, args.min_qual, args.max_qual, args.max_size, args.sv_threshold,
            args.phase_threshold, args.credit_threshold, b2s(getattr(args, "realign_truth", False)), b2s(getattr(args, "realign_query", False)),
            b2s(getattr(args, "realign_only", False)), args.cluster, args.cluster_gap,
            args.reach_min_gap, args.max_iterations, 64, 64.0, args.sub, args.open, args.extend,
            getattr(args, "eval_sub", 3), getattr(args, "eval_open", 2), getattr(args, "eval_extend", 1), b2s(getattr(args, "distance", False))))
    with open(prefix + "parameters.txt", "w") as f:
        f.write(text)


class VrpVcfContig(C.Structure):
    _fields_ = [("name", C.c_char_p), ("length", C.c_int32), ("ploidy", C.c_int32), ("seq", A.P_u8), ("seq_len", C.c_int64),
                ("hap", VrpHap * 2)]


def write_vcf(path, callset, fasta=None, vars=None, file_date=None):
    """a callset as a VCF (variantData::write_vcf, variant.cpp:132-222; vrp_write_vcf).  callset: what vcfdist_amd.io.read_vcf returns
    (contigs, lengths, ploidy, sample, vars); vars: per-contig [hap 1, hap 2] column dicts in place of callset["vars"] (a realigned
    callset); fasta: {name: sequence} for the anchor bases of INS / DEL records"""
    vars = callset["vars"] if vars is None else vars
    keep = []

    def own(a, dt):
        a = np.ascontiguousarray(a, dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep.append(a)
        return A._ptr(a, np.ctypeslib.as_ctypes_type(dt))
    n = len(callset["contigs"])
    arr = (VrpVcfContig * max(n, 1))()
    for k, name in enumerate(callset["contigs"]):
        c = arr[k]
        nm = name.encode()
        keep.append(nm)
        c.name, c.length, c.ploidy = nm, int(callset["lengths"][k]), int(callset["ploidy"][k])
        if fasta is not None and name in fasta:
            sq = np.asarray(fasta[name], np.uint8)
            c.seq, c.seq_len = own(sq, np.uint8), len(sq)
        for h in range(2):
            s, H = vars[k][h], c.hap[h]
            H.n_var = len(s["pos"])
            H.pos, H.type, H.var_qual = own(s["pos"], np.int32), own(s["type"], np.uint8), own(s["var_qual"], np.float32)
            H.ref_len, H.alt_len = own(s["ref_len"], np.int32), own(s["alt_len"], np.int32)
            H.ref_off, H.alt_off, H.pool = own(s["ref_off"], np.int64), own(s["alt_off"], np.int64), own(s["pool"], np.uint8)
    L = api.lib()
    L.vrp_write_vcf.argtypes = [C.c_char_p, C.POINTER(VrpVcfContig), C.c_int32, C.c_char_p, C.c_char_p]
    _check(L.vrp_write_vcf(path.encode(), arr, n, callset["sample"].encode(), file_date.encode() if file_date else None), "vrp_write_vcf")
