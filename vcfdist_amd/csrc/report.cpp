// report.cpp -- the output tables behind the precision/recall path (include/vcfdist_report.h): host formatting of the
// device results into the reference's files.  Every format string follows the reference's fprintf at the cited line
// so that the files compare byte for byte; the control flow is organised around one merge iterator per file instead
// of the reference's per-haplotype copies.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vcfdist_pr.h"
#include "../../include/vcfdist_report.h"
#include "../../include/vcfdist_bootstrap.h"
#include "../../include/vcfdist_varstrata.h"
#include "../../include/vcfdist_derive.h"
#include "../../include/vcfdist_errclass.h"
#include "../../include/vcfdist_matchkind.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }

// string tables of src/main.cpp:14-24
const char *const TYPE_STR[] = {"REF", "SNP", "INS", "DEL", "CPX"};
const char *const VARTYPE_STR[] = {"SNP", "INDEL", "SV", "ALL"};
const char *const ERROR_STR[] = {"TP", "FP", "FN", "PE", "GE", "??"};
const char *const REGION_STR[] = {"OUTSIDE", "INSIDE ", "BORDER ", "OFF CTG"};
const char *const PHASE_STR[] = {"=", "X", "?"};

struct File {
    FILE *f = nullptr;
    explicit File(const char *path) { if (path) f = fopen(path, "w"); }
    ~File() { if (f) fclose(f); }
    operator FILE *() const { return f; }
    // flush and close now; false if any write failed (disk full, ...): the caller reports it instead of VRP_OK
    bool finish() {
        if (!f) return false;
        const bool bad = fflush(f) != 0 || ferror(f) != 0;
        const bool closed = fclose(f) == 0;
        f = nullptr;
        return !bad && closed;
    }
};

struct Metrics { int query_tp, query_fp, truth_tp, truth_fn; float precision, recall, f1, f1_q; };

Metrics metrics(const int64_t *counts, int nq, int type, int qidx) {
    auto at = [&](int callset, int err) { return int(counts[((size_t(callset) * VPR_VARTYPES + type) * 3 + err) * nq + qidx]); };
    Metrics m;
    m.query_tp = at(0, VPR_ERRTYPE_TP); m.query_fp = at(0, VPR_ERRTYPE_FP);
    m.truth_tp = at(1, VPR_ERRTYPE_TP); m.truth_fn = at(1, VPR_ERRTYPE_FN);
    const int query_tot = m.query_tp + m.query_fp, truth_tot = m.truth_tp + m.truth_fn;
    m.precision = query_tot == 0 ? 1 : float(m.query_tp) / query_tot;
    m.recall = truth_tot == 0 ? 1 : float(m.truth_tp) / truth_tot;
    m.f1 = m.precision + m.recall > 0 ? 2 * m.precision * m.recall / (m.precision + m.recall) : 0;
    m.f1_q = float(std::min(100.0, std::max(0.0, -10 * std::log10(double(1 - m.f1)))));   // qscore(), edit.cpp:102
    return m;
}

// the evaluation (ORIG / SWAP) a supercluster's variants are reported under: print.cpp:699-704
inline int swap_of(const vrp_contig &c, int sci) {
    const int p = c.sc_phase[sci];
    return p == VPR_PHASE_ORIG ? 0 : p == VPR_PHASE_SWAP ? 1 : (c.pb_phase[sci] != 0);
}

bool contig_ok(const vrp_contig &c) {
    if (!c.name) return false;
    if (c.n_sc > 0 && (!c.sc_beg || !c.sc_end || !c.sc_phase || !c.pb_phase)) return false;
    for (int i = 0; i < 4; i++) {
        const vrp_hap &h = c.hap[i];
        if (h.n_var > 0 && (!h.pos || !h.type || !h.cluster_beg || !h.pool || !h.ref_len || !h.alt_len || !h.ref_off || !h.alt_off))
            return false;
    }
    return true;
}

}  // namespace

extern "C" const char *vrp_last_error(void) { return g_err.c_str(); }

extern "C" int32_t vrp_phase_blocks(const int32_t *sc_phase_set, int32_t n_sc, int32_t *phase_block) {
    if (n_sc < 0 || !phase_block || (n_sc && !sc_phase_set)) return VRP_ERR_ARG;
    int32_t n_pb = 0, cur = -1;   // a new block wherever the phase set changes (phase.cpp:249-258)
    for (int32_t k = 0; k < n_sc; k++)
        if (sc_phase_set[k] != cur) { phase_block[n_pb++] = k; cur = sc_phase_set[k]; }
    phase_block[n_pb] = n_sc;
    return n_pb;
}

namespace {
// the BEST threshold of one type: the first quality of the largest F1 (print.cpp:470), as pr_rows settles it
int best_qual_of(const int64_t *counts, int type, int min_qual, int max_qual) {
    const int nq = max_qual - min_qual + 1;
    float best = 0;
    int best_qual = 0;
    for (int qual = min_qual; qual <= max_qual; qual++) {
        const Metrics m = metrics(counts, nq, type, qual - min_qual);
        if (m.f1 > best) { best = m.f1; best_qual = qual; }
    }
    // (an all-zero F1 column leaves quality 0 in the reference, which it then indexes; keep the index in range)
    return best_qual < min_qual || best_qual > max_qual ? min_qual : best_qual;
}

// the rows of precision-recall.tsv (all) and precision-recall-summary.tsv (sum) for one set of counters, every line behind
// `lead` ("" for the unstratified files, "<stratum>\t" for the stratified ones)
void pr_rows(FILE *all, FILE *sum, const char *lead, const int64_t *counts, int min_qual, int max_qual) {
    const int nq = max_qual - min_qual + 1;
    int best_qual[VPR_VARTYPES];
    for (int type = 0; type < VPR_VARTYPES; type++) {
        for (int qual = min_qual; qual <= max_qual; qual++) {
            const Metrics m = metrics(counts, nq, type, qual - min_qual);
            fprintf(all, "%s%s\t%d\t%f\t%f\t%f\t%f\t%d\t%d\t%d\t%d\t%d\t%d\n", lead, VARTYPE_STR[type], qual, m.precision, m.recall,
                    m.f1, m.f1_q, m.truth_tp + m.truth_fn, m.truth_tp, m.truth_fn, m.query_tp + m.query_fp, m.query_tp, m.query_fp);
        }
        best_qual[type] = best_qual_of(counts, type, min_qual, max_qual);
    }
    for (int type = 0; type < VPR_VARTYPES; type++) {
        const int quals[2] = {min_qual, best_qual[type]};
        const char *const thresh[2] = {"NONE", "BEST"};
        for (int i = 0; i < 2; i++) {
            const Metrics m = metrics(counts, nq, type, quals[i] - min_qual);
            fprintf(sum, "%s%s\t%s\t%d\t%d\t%d\t%d\t%d\t%f\t%f\t%f\t%f\n", lead, VARTYPE_STR[type], thresh[i], quals[i], m.truth_tp,
                    m.query_tp, m.truth_fn, m.query_fp, m.precision, m.recall, m.f1, m.f1_q);
        }
    }
}
// the rows of bootstrap-precision-recall-summary.tsv (sum) and, where wanted, bootstrap-replicates.tsv (rep) for one set of
// point counters and its n_rep replicate counters (include/vcfdist_bootstrap.h: percentile interval, BEST fixed at the point
// estimate's quality), every summary line behind `lead`
void boot_rows(FILE *sum, FILE *rep, const char *lead, const int64_t *counts, const int64_t *counts_boot, int n_rep,
               unsigned long long seed, int min_qual, int max_qual) {
    const int nq = max_qual - min_qual + 1;
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(nq);
    const char *const thresh[2] = {"NONE", "BEST"};
    int quals[VPR_VARTYPES][2];
    for (int type = 0; type < VPR_VARTYPES; type++) { quals[type][0] = min_qual; quals[type][1] = best_qual_of(counts, type, min_qual, max_qual); }
    // x[floor(0.025 n)] and x[ceil(0.975 n) - 1] in integers: n / 40 and ceil(39 n / 40) - 1
    const size_t lo = size_t(n_rep) / 40, hi = (size_t(39) * size_t(n_rep) + 39) / 40 - 1;
    std::vector<float> x[3];
    for (int type = 0; type < VPR_VARTYPES; type++)
        for (int i = 0; i < 2; i++) {
            const Metrics m = metrics(counts, nq, type, quals[type][i] - min_qual);
            for (auto &v : x) v.resize(size_t(n_rep));
            for (int r = 0; r < n_rep; r++) {
                const Metrics b = metrics(counts_boot + size_t(r) * nc1, nq, type, quals[type][i] - min_qual);
                x[0][size_t(r)] = b.precision; x[1][size_t(r)] = b.recall; x[2][size_t(r)] = b.f1;
            }
            for (auto &v : x) std::sort(v.begin(), v.end());
            fprintf(sum, "%s%s\t%s\t%d\t%d\t%llu\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", lead, VARTYPE_STR[type], thresh[i], quals[type][i],
                    n_rep, seed, m.precision, x[0][lo], x[0][hi], m.recall, x[1][lo], x[1][hi], m.f1, x[2][lo], x[2][hi]);
        }
    if (!rep) return;
    for (int r = 0; r < n_rep; r++)
        for (int type = 0; type < VPR_VARTYPES; type++)
            for (int i = 0; i < 2; i++) {
                const Metrics b = metrics(counts_boot + size_t(r) * nc1, nq, type, quals[type][i] - min_qual);
                fprintf(rep, "%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%f\t%f\t%f\n", r, VARTYPE_STR[type], thresh[i], quals[type][i], b.truth_tp,
                        b.query_tp, b.truth_fn, b.query_fp, b.precision, b.recall, b.f1);
            }
}
const char *const BOOT_SUM_HEADER = "VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tREPLICATES\tSEED\tPREC\tPREC_LO\tPREC_HI\tRECALL\tRECALL_LO\tRECALL_HI\tF1_SCORE\tF1_LO\tF1_HI\n";
const char *const BOOT_REP_HEADER = "REPLICATE\tVAR_TYPE\tTHRESHOLD\tMIN_QUAL\tTRUTH_TP\tQUERY_TP\tTRUTH_FN\tQUERY_FP\tPREC\tRECALL\tF1_SCORE\n";
const char *const PR_ALL_HEADER = "VAR_TYPE\tMIN_QUAL\tPREC\tRECALL\tF1_SCORE\tF1_QSCORE\tTRUTH_TOTAL\tTRUTH_TP\tTRUTH_FN\tQUERY_TOTAL\tQUERY_TP\tQUERY_FP\n";
const char *const PR_SUM_HEADER = "VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tTRUTH_TP\tQUERY_TP\tTRUTH_FN\tQUERY_FP\tPREC\tRECALL\tF1_SCORE\tF1_QSCORE\n";
}  // namespace

extern "C" int vrp_write_precision_recall(const char *prefix, const int64_t *counts, int32_t min_qual, int32_t max_qual) {
    if (!prefix || !counts || max_qual < min_qual) return fail(VRP_ERR_ARG, "vrp_write_precision_recall: bad argument");
    const std::string fn_all = std::string(prefix) + "precision-recall.tsv", fn_sum = std::string(prefix) + "precision-recall-summary.tsv";
    File all(fn_all.c_str());
    if (!all) return fail(VRP_ERR_OPEN, "cannot create " + fn_all);
    File sum(fn_sum.c_str());
    if (!sum) return fail(VRP_ERR_OPEN, "cannot create " + fn_sum);
    fputs(PR_ALL_HEADER, all);
    fputs(PR_SUM_HEADER, sum);
    pr_rows(all, sum, "", counts, min_qual, max_qual);
    if (!all.finish() || !sum.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn_all + " / " + fn_sum);
    return VRP_OK;
}

extern "C" int vrp_write_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *counts,
                                    int32_t min_qual, int32_t max_qual) {
    if (!prefix || !names || n_strata < 0 || (n_strata && !counts) || max_qual < min_qual) return fail(VRP_ERR_ARG, "vrp_write_stratified: bad argument");
    for (int32_t k = 0; k < n_strata; k++) if (!names[k]) return fail(VRP_ERR_ARG, "vrp_write_stratified: null stratum name");
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(max_qual - min_qual + 1);
    const std::string fn_all = std::string(prefix) + "stratified-precision-recall.tsv",
                      fn_sum = std::string(prefix) + "stratified-precision-recall-summary.tsv";
    File all(fn_all.c_str());
    if (!all) return fail(VRP_ERR_OPEN, "cannot create " + fn_all);
    File sum(fn_sum.c_str());
    if (!sum) return fail(VRP_ERR_OPEN, "cannot create " + fn_sum);
    fprintf(all, "STRATUM\t%s", PR_ALL_HEADER);
    fprintf(sum, "STRATUM\t%s", PR_SUM_HEADER);
    for (int32_t k = 0; k < n_strata; k++)
        pr_rows(all, sum, (std::string(names[k]) + "\t").c_str(), counts + size_t(k) * nc1, min_qual, max_qual);
    if (!all.finish() || !sum.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn_all + " / " + fn_sum);
    return VRP_OK;
}

// context-strata.bed, repeat-strata.bed, long-repeat-strata.bed and near-repeat-strata.bed: one body
static int write_strata_bed(const char *entry, const char *file, const char *prefix, const char *const *contigs, int32_t n_ctg,
                            const char *const *names, int32_t n_strata, const int64_t *iv_off, const int32_t *start, const int32_t *stop) {
    const std::string who = entry;
    if (!prefix || !contigs || !names || n_ctg < 0 || n_strata < 0 || !iv_off) return fail(VRP_ERR_ARG, who + ": bad argument");
    const size_t n_rows = size_t(n_ctg) * size_t(n_strata);
    if (iv_off[n_rows] > iv_off[0] && (!start || !stop)) return fail(VRP_ERR_ARG, who + ": null interval table");
    for (int32_t c = 0; c < n_ctg; c++) if (!contigs[c]) return fail(VRP_ERR_ARG, who + ": null contig name");
    for (int32_t k = 0; k < n_strata; k++) if (!names[k]) return fail(VRP_ERR_ARG, who + ": null stratum name");
    const std::string fn = std::string(prefix) + file;
    File bed(fn.c_str());
    if (!bed) return fail(VRP_ERR_OPEN, "cannot create " + fn);
    for (size_t r = 0; r < n_rows; r++)
        for (int64_t j = iv_off[r]; j < iv_off[r + 1]; j++)
            fprintf(bed, "%s\t%d\t%d\t%s\n", contigs[r / size_t(n_strata)], start[j], stop[j], names[r % size_t(n_strata)]);
    if (!bed.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn);
    return VRP_OK;
}

extern "C" int vrp_write_context_bed(const char *prefix, const char *const *contigs, int32_t n_ctg, const char *const *names, int32_t n_strata,
                                     const int64_t *iv_off, const int32_t *start, const int32_t *stop) {
    return write_strata_bed("vrp_write_context_bed", "context-strata.bed", prefix, contigs, n_ctg, names, n_strata, iv_off, start, stop);
}

extern "C" int vrp_write_repeat_bed(const char *prefix, const char *const *contigs, int32_t n_ctg, const char *const *names, int32_t n_strata,
                                    const int64_t *iv_off, const int32_t *start, const int32_t *stop) {
    return write_strata_bed("vrp_write_repeat_bed", "repeat-strata.bed", prefix, contigs, n_ctg, names, n_strata, iv_off, start, stop);
}

extern "C" int vrp_write_long_repeat_bed(const char *prefix, const char *const *contigs, int32_t n_ctg, const char *const *names, int32_t n_strata,
                                         const int64_t *iv_off, const int32_t *start, const int32_t *stop) {
    return write_strata_bed("vrp_write_long_repeat_bed", "long-repeat-strata.bed", prefix, contigs, n_ctg, names, n_strata, iv_off, start, stop);
}

extern "C" int vrp_write_near_repeat_bed(const char *prefix, const char *const *contigs, int32_t n_ctg, const char *const *names, int32_t n_strata,
                                         const int64_t *iv_off, const int32_t *start, const int32_t *stop) {
    return write_strata_bed("vrp_write_near_repeat_bed", "near-repeat-strata.bed", prefix, contigs, n_ctg, names, n_strata, iv_off, start, stop);
}

extern "C" int vrp_write_variant_strata(const char *prefix, const char *const *names, const vpr_variant_stratum *spec, int32_t n_spec,
                                        const int64_t *n_query, const int64_t *n_truth) {
    if (!prefix || !names || !spec || n_spec < 0 || !n_query || !n_truth) return fail(VRP_ERR_ARG, "vrp_write_variant_strata: bad argument");
    static const char *const KIND[] = {"SIZE", "TI", "TV", "HOM", "HET", "NEAR"};
    for (int32_t k = 0; k < n_spec; k++) {
        if (!names[k]) return fail(VRP_ERR_ARG, "vrp_write_variant_strata: null stratum name");
        if (spec[k].kind < VPR_VS_SIZE || spec[k].kind > VPR_VS_NEAR) return fail(VRP_ERR_ARG, "vrp_write_variant_strata: unknown kind");
    }
    const std::string fn = std::string(prefix) + "variant-strata.tsv";
    File out(fn.c_str());
    if (!out) return fail(VRP_ERR_OPEN, "cannot create " + fn);
    fputs("STRATUM\tKIND\tTYPE\tMIN_LEN\tMAX_LEN\tWINDOW\tMIN_N\tMAX_N\tQUERY_VARS\tTRUTH_VARS\n", out);
    auto num = [](bool set, int32_t x) { return set ? std::to_string(x) : std::string("."); };      // '.': no such parameter, or an open bound
    for (int32_t k = 0; k < n_spec; k++) {
        const vpr_variant_stratum &s = spec[k];
        const bool size = s.kind == VPR_VS_SIZE, near = s.kind == VPR_VS_NEAR;
        fprintf(out, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%lld\t%lld\n", names[k], KIND[s.kind], size ? TYPE_STR[s.type == VPR_TYPE_INS ? 2 : 3] : ".",
                num(size, s.min_len).c_str(), num(size && s.max_len != 0, s.max_len).c_str(), num(near, s.window).c_str(), num(near, s.min_n).c_str(),
                num(near && s.max_n >= 0, s.max_n).c_str(), (long long)n_query[k], (long long)n_truth[k]);
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn);
    return VRP_OK;
}

extern "C" int vrp_write_derived_strata(const char *prefix, const char *const *names, const int32_t *kind, const char *const *expression, int32_t n,
                                        const int64_t *n_query, const int64_t *n_truth) {
    if (!prefix || !names || !kind || !expression || n < 0 || !n_query || !n_truth) return fail(VRP_ERR_ARG, "vrp_write_derived_strata: bad argument");
    for (int32_t k = 0; k < n; k++) {
        if (!names[k] || !expression[k]) return fail(VRP_ERR_ARG, "vrp_write_derived_strata: null stratum name or expression");
        if (kind[k] != VPR_DV_KIND_DERIVE && kind[k] != VPR_DV_KIND_CROSS) return fail(VRP_ERR_ARG, "vrp_write_derived_strata: unknown kind");
    }
    const std::string fn = std::string(prefix) + "derived-strata.tsv";
    File out(fn.c_str());
    if (!out) return fail(VRP_ERR_OPEN, "cannot create " + fn);
    fputs("NAME\tKIND\tEXPRESSION\tQUERY_MEMBERS\tTRUTH_MEMBERS\n", out);
    for (int32_t k = 0; k < n; k++)
        fprintf(out, "%s\t%s\t%s\t%lld\t%lld\n", names[k], kind[k] == VPR_DV_KIND_CROSS ? "cross" : "derive", expression[k], (long long)n_query[k],
                (long long)n_truth[k]);
    if (!out.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn);
    return VRP_OK;
}

// The files of a label pass (a feature that counts a label per variant: include/vcfdist_errclass.h, vcfdist_matchkind.h).  counts
// [2][VPR_VARTYPES][stride][nq]; a row's cells are each callset's total, then its first n_labels[callset] labels, under `cols`
namespace {
struct LabelTable { const char *stem, *cols; int n_labels[2]; int stride; };
const LabelTable EC_TABLE = {"error-classes",
                             "QUERY_FP\tFP_GT\tFP_SYNC\tFP_PHASE\tFP_SITE\tFP_NEAR\tFP_ALONE\tTRUTH_FN\tFN_GT\tFN_SYNC\tFN_PHASE\tFN_SITE\tFN_NEAR\tFN_ALONE\tFN_LOWQ\n",
                             {VPR_EC_CLASSES - 1, VPR_EC_CLASSES}, VPR_EC_CLASSES};      // (the query has no LOWQ)
const LabelTable MK_TABLE = {"match-kinds", "QUERY_TP\tQTP_EXACT\tQTP_SHIFTED\tQTP_REGROUPED\tQTP_PARTIAL\tTRUTH_TP\tTTP_EXACT\tTTP_SHIFTED\tTTP_REGROUPED\tTTP_PARTIAL\n",
                             {VPR_MK_KINDS, VPR_MK_KINDS}, VPR_MK_KINDS};

// the cells of one row (type, threshold index k), in column order
void label_cells(const LabelTable &T, const int64_t *counts, int nq, int type, int k, std::vector<long long> *out) {
    out->clear();
    for (int cs = 0; cs < 2; cs++) {
        const int64_t *c = counts + (size_t(cs) * VPR_VARTYPES + type) * T.stride * size_t(nq) + k;
        long long tot = 0;
        for (int j = 0; j < T.n_labels[cs]; j++) tot += c[size_t(j) * nq];
        out->push_back(tot);
        for (int j = 0; j < T.n_labels[cs]; j++) out->push_back((long long)c[size_t(j) * nq]);
    }
}

// the rows of <stem>.tsv (a row per type and threshold) and <stem>-summary.tsv (the NONE and BEST rows of each type, BEST from
// pr_counts by vpr_pr_summary's rule) for one set of label counts, every line behind `lead`
void label_rows(FILE *all, FILE *sum, const char *lead, const LabelTable &T, const int64_t *counts, const int64_t *pr_counts, int min_qual,
                int max_qual) {
    const int nq = max_qual - min_qual + 1;
    std::vector<long long> row;
    auto cells = [&](FILE *f, int type, int k) {
        label_cells(T, counts, nq, type, k, &row);
        for (size_t j = 0; j < row.size(); j++) fprintf(f, "%s%lld", j ? "\t" : "", row[j]);
        fputc('\n', f);
    };
    for (int type = 0; type < VPR_VARTYPES; type++)
        for (int qual = min_qual; qual <= max_qual; qual++) {
            fprintf(all, "%s%s\t%d\t", lead, VARTYPE_STR[type], qual);
            cells(all, type, qual - min_qual);
        }
    for (int type = 0; type < VPR_VARTYPES; type++) {
        const int quals[2] = {min_qual, best_qual_of(pr_counts, type, min_qual, max_qual)};
        const char *const thresh[2] = {"NONE", "BEST"};
        for (int i = 0; i < 2; i++) {
            fprintf(sum, "%s%s\t%s\t%d\t", lead, VARTYPE_STR[type], thresh[i], quals[i]);
            cells(sum, type, quals[i] - min_qual);
        }
    }
}

// <stem>.tsv and <stem>-summary.tsv (names null), or stratified-<stem>.tsv and stratified-<stem>-summary.tsv: the same two
// tables once per stratum behind a leading STRATUM column, counts[n_strata][...] and pr_counts[n_strata][...] (vpr_pr_counts_strata)
int write_label_counts(const char *entry, const char *prefix, const LabelTable &T, const char *const *names, int32_t n_strata,
                       const int64_t *counts, const int64_t *pr_counts, int32_t min_qual, int32_t max_qual) {
    if (!prefix || max_qual < min_qual || (names ? n_strata < 0 || (n_strata && (!counts || !pr_counts)) : !counts || !pr_counts))
        return fail(VRP_ERR_ARG, std::string(entry) + ": bad argument");
    for (int32_t k = 0; names && k < n_strata; k++) if (!names[k]) return fail(VRP_ERR_ARG, std::string(entry) + ": null stratum name");
    const int nq = max_qual - min_qual + 1;
    const std::string head = std::string(prefix) + (names ? "stratified-" : "") + T.stem;
    const std::string fn_all = head + ".tsv", fn_sum = head + "-summary.tsv";
    File all(fn_all.c_str());
    if (!all) return fail(VRP_ERR_OPEN, "cannot create " + fn_all);
    File sum(fn_sum.c_str());
    if (!sum) return fail(VRP_ERR_OPEN, "cannot create " + fn_sum);
    fprintf(all, "%sVAR_TYPE\tMIN_QUAL\t%s", names ? "STRATUM\t" : "", T.cols);
    fprintf(sum, "%sVAR_TYPE\tTHRESHOLD\tMIN_QUAL\t%s", names ? "STRATUM\t" : "", T.cols);
    if (!names) {
        label_rows(all, sum, "", T, counts, pr_counts, min_qual, max_qual);
    } else {
        const size_t nl1 = size_t(2) * VPR_VARTYPES * T.stride * size_t(nq), nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(nq);
        for (int32_t k = 0; k < n_strata; k++)
            label_rows(all, sum, (std::string(names[k]) + "\t").c_str(), T, counts + size_t(k) * nl1, pr_counts + size_t(k) * nc1, min_qual, max_qual);
    }
    if (!all.finish() || !sum.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn_all + " / " + fn_sum);
    return VRP_OK;
}

// bootstrap-<stem>-summary.tsv: the rows of <stem>-summary.tsv, every count column followed by its _LO and _HI -- the replicate
// counts sorted as integers, x[floor(0.025 n)] and x[ceil(0.975 n) - 1]; BEST's quality is the point estimate's
int write_label_bootstrap(const char *entry, const char *prefix, const LabelTable &T, const int64_t *counts, const int64_t *pr_counts,
                          const int64_t *boot, int32_t n_rep, int32_t min_qual, int32_t max_qual) {
    if (!prefix || !counts || !pr_counts || !boot || n_rep < 1 || max_qual < min_qual) return fail(VRP_ERR_ARG, std::string(entry) + ": bad argument");
    const int nq = max_qual - min_qual + 1;
    const size_t nl1 = size_t(2) * VPR_VARTYPES * T.stride * size_t(nq);
    const std::string fn = std::string(prefix) + "bootstrap-" + T.stem + "-summary.tsv";
    File sum(fn.c_str());
    if (!sum) return fail(VRP_ERR_OPEN, "cannot create " + fn);
    fputs("VAR_TYPE\tTHRESHOLD\tMIN_QUAL", sum);
    for (const char *p = T.cols; *p && *p != '\n';) {
        const char *e = p;
        while (*e != '\t' && *e != '\n') e++;
        const std::string col(p, e);
        fprintf(sum, "\t%s\t%s_LO\t%s_HI", col.c_str(), col.c_str(), col.c_str());
        p = *e == '\t' ? e + 1 : e;
    }
    fputc('\n', sum);
    const size_t lo = size_t(n_rep) / 40, hi = (size_t(39) * size_t(n_rep) + 39) / 40 - 1;
    std::vector<long long> point, row;
    std::vector<std::vector<long long>> x;
    for (int type = 0; type < VPR_VARTYPES; type++) {
        const int quals[2] = {min_qual, best_qual_of(pr_counts, type, min_qual, max_qual)};
        const char *const thresh[2] = {"NONE", "BEST"};
        for (int i = 0; i < 2; i++) {
            label_cells(T, counts, nq, type, quals[i] - min_qual, &point);
            x.assign(point.size(), std::vector<long long>(size_t(n_rep)));
            for (int r = 0; r < n_rep; r++) {
                label_cells(T, boot + size_t(r) * nl1, nq, type, quals[i] - min_qual, &row);
                for (size_t j = 0; j < row.size(); j++) x[j][size_t(r)] = row[j];
            }
            fprintf(sum, "%s\t%s\t%d", VARTYPE_STR[type], thresh[i], quals[i]);
            for (size_t j = 0; j < point.size(); j++) {
                std::sort(x[j].begin(), x[j].end());
                fprintf(sum, "\t%lld\t%lld\t%lld", point[j], x[j][lo], x[j][hi]);
            }
            fputc('\n', sum);
        }
    }
    if (!sum.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn);
    return VRP_OK;
}
}  // namespace

extern "C" int vrp_write_error_classes(const char *prefix, const int64_t *class_counts, const int64_t *pr_counts, int32_t min_qual,
                                       int32_t max_qual) {
    return write_label_counts("vrp_write_error_classes", prefix, EC_TABLE, nullptr, 0, class_counts, pr_counts, min_qual, max_qual);
}

extern "C" int vrp_write_match_kinds(const char *prefix, const int64_t *kind_counts, const int64_t *pr_counts, int32_t min_qual,
                                     int32_t max_qual) {
    return write_label_counts("vrp_write_match_kinds", prefix, MK_TABLE, nullptr, 0, kind_counts, pr_counts, min_qual, max_qual);
}

extern "C" int vrp_write_error_classes_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *class_counts,
                                                  const int64_t *pr_counts, int32_t min_qual, int32_t max_qual) {
    if (!names) return fail(VRP_ERR_ARG, "vrp_write_error_classes_stratified: bad argument");
    return write_label_counts("vrp_write_error_classes_stratified", prefix, EC_TABLE, names, n_strata, class_counts, pr_counts, min_qual, max_qual);
}

extern "C" int vrp_write_match_kinds_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *kind_counts,
                                                const int64_t *pr_counts, int32_t min_qual, int32_t max_qual) {
    if (!names) return fail(VRP_ERR_ARG, "vrp_write_match_kinds_stratified: bad argument");
    return write_label_counts("vrp_write_match_kinds_stratified", prefix, MK_TABLE, names, n_strata, kind_counts, pr_counts, min_qual, max_qual);
}

extern "C" int vrp_write_error_classes_bootstrap(const char *prefix, const int64_t *class_counts, const int64_t *pr_counts,
                                                 const int64_t *class_boot, int32_t n_rep, int32_t min_qual, int32_t max_qual) {
    return write_label_bootstrap("vrp_write_error_classes_bootstrap", prefix, EC_TABLE, class_counts, pr_counts, class_boot, n_rep, min_qual, max_qual);
}

extern "C" int vrp_write_match_kinds_bootstrap(const char *prefix, const int64_t *kind_counts, const int64_t *pr_counts, const int64_t *kind_boot,
                                               int32_t n_rep, int32_t min_qual, int32_t max_qual) {
    return write_label_bootstrap("vrp_write_match_kinds_bootstrap", prefix, MK_TABLE, kind_counts, pr_counts, kind_boot, n_rep, min_qual, max_qual);
}

extern "C" int vrp_write_bootstrap(const char *prefix, const int64_t *counts, const int64_t *counts_boot, int32_t n_rep, uint64_t seed,
                                   int32_t min_qual, int32_t max_qual) {
    if (!prefix || !counts || !counts_boot || n_rep < 1 || max_qual < min_qual) return fail(VRP_ERR_ARG, "vrp_write_bootstrap: bad argument");
    const std::string fn_sum = std::string(prefix) + "bootstrap-precision-recall-summary.tsv", fn_rep = std::string(prefix) + "bootstrap-replicates.tsv";
    File sum(fn_sum.c_str());
    if (!sum) return fail(VRP_ERR_OPEN, "cannot create " + fn_sum);
    File rep(fn_rep.c_str());
    if (!rep) return fail(VRP_ERR_OPEN, "cannot create " + fn_rep);
    fputs(BOOT_SUM_HEADER, sum);
    fputs(BOOT_REP_HEADER, rep);
    boot_rows(sum, rep, "", counts, counts_boot, n_rep, seed, min_qual, max_qual);
    if (!sum.finish() || !rep.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn_sum + " / " + fn_rep);
    return VRP_OK;
}

extern "C" int vrp_write_bootstrap_stratified(const char *prefix, const char *const *names, int32_t n_strata, const int64_t *counts,
                                              const int64_t *counts_boot, int32_t n_rep, uint64_t seed, int32_t min_qual, int32_t max_qual) {
    if (!prefix || !names || n_strata < 0 || (n_strata && (!counts || !counts_boot)) || n_rep < 1 || max_qual < min_qual)
        return fail(VRP_ERR_ARG, "vrp_write_bootstrap_stratified: bad argument");
    for (int32_t k = 0; k < n_strata; k++) if (!names[k]) return fail(VRP_ERR_ARG, "vrp_write_bootstrap_stratified: null stratum name");
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(max_qual - min_qual + 1);
    const std::string fn_sum = std::string(prefix) + "stratified-bootstrap-precision-recall-summary.tsv";
    File sum(fn_sum.c_str());
    if (!sum) return fail(VRP_ERR_OPEN, "cannot create " + fn_sum);
    fprintf(sum, "STRATUM\t%s", BOOT_SUM_HEADER);
    for (int32_t k = 0; k < n_strata; k++)
        boot_rows(sum, nullptr, (std::string(names[k]) + "\t").c_str(), counts + size_t(k) * nc1, counts_boot + size_t(k) * size_t(n_rep) * nc1,
                  n_rep, seed, min_qual, max_qual);
    if (!sum.finish()) return fail(VRP_ERR_OPEN, "write error on " + fn_sum);
    return VRP_OK;
}

extern "C" int vrp_write_phase_blocks(const char *path, const vrp_contig *ctgs, int32_t n_ctg) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs)) return fail(VRP_ERR_ARG, "vrp_write_phase_blocks: bad argument");
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "CONTIG\tPHASE_BLOCK\tSTART\tSTOP\tSIZE\tSUPERCLUSTERS\tFLIP_ERRORS\tSWITCH_ERRORS\n");
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_contig &c = ctgs[ci];
        if (!contig_ok(c) || (c.n_pb > 0 && !c.phase_block)) return fail(VRP_ERR_ARG, "vrp_write_phase_blocks: incomplete contig");
        for (int32_t i = 0; i < c.n_pb && c.n_sc > 0; i++) {
            const int32_t first = c.phase_block[i], last = c.phase_block[i + 1] - 1;
            // errors strictly inside the block: an event on its first supercluster belongs to the border (print.cpp:596-603)
            auto inside = [&](const int32_t *ev, int32_t n) {
                int32_t k = 0;
                for (int32_t e = 0; e < n; e++) k += ev[e] > first && ev[e] <= last;
                return k;
            };
            const int32_t beg = c.sc_beg[first], end = c.sc_end[last];
            fprintf(out, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", c.name, i, beg, end, end - beg, last - first + 1,
                    inside(c.flips, c.n_flips), inside(c.switches, c.n_switches));
        }
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}

// ---- phasing errors: switchflips.tsv (phaseblockData::write_switchflips, phase.cpp:406-509), phasing-summary.tsv
// (write_phasing_summary, phase.cpp:515-528) and the three NG50 figures behind it (calculate_ng50, phase.cpp:534-626).
// All of them sweep a contig's superclusters from break to break.  A break is the start of a phase block (a new phase
// set: not an error), a switch error or a flip error; the next one is the pending event with the smallest supercluster,
// where on equal superclusters a flip takes precedence over a switch error over a block start -- and a flip that is met
// while a block start is the candidate is reported as "switch + flip" and uses up that block start, wherever the block
// start lies (the reference's comparison order; the tables must come out the same).
namespace {
enum { BRK_FLIP = 0, BRK_BLOCK = 1, BRK_BLOCK_FLIP = 2, BRK_SWITCH_ERR = 3, BRK_NONE = 6 };

// f(kind, supercluster, index of the phase block the break is counted in); false = events out of order
template <class F>
bool for_each_break(const vrp_contig &c, bool with_switches, bool with_flips, F f) {
    int32_t i_pb = 1, i_sw = 0, i_fl = 0, at = 0;
    for (;;) {
        int kind = BRK_NONE;
        int32_t nxt = c.n_sc;
        if (i_pb < c.n_pb && c.phase_block[i_pb] <= nxt) { kind = BRK_BLOCK; nxt = c.phase_block[i_pb]; }
        if (with_switches && i_sw < c.n_switches && c.switches[i_sw] <= nxt) { kind = BRK_SWITCH_ERR; nxt = c.switches[i_sw]; }
        if (with_flips && i_fl < c.n_flips && c.flips[i_fl] <= nxt) { kind = kind == BRK_BLOCK ? BRK_BLOCK_FLIP : BRK_FLIP; nxt = c.flips[i_fl]; }
        if (kind == BRK_NONE) return true;
        if (nxt <= at) return false;        // the reference's ERROR("Next supercluster ... is not after current supercluster")
        f(kind, nxt, i_pb - 1);
        if (kind == BRK_FLIP || kind == BRK_BLOCK_FLIP) i_fl++;
        if (kind == BRK_BLOCK || kind == BRK_BLOCK_FLIP) i_pb++;
        if (kind == BRK_SWITCH_ERR) i_sw++;
        at = nxt;
    }
}

bool phasing_ok(const vrp_contig &c) {
    if (!contig_ok(c) || c.n_pb < 0 || c.n_switches < 0 || c.n_flips < 0) return false;
    if (c.n_sc > 0 && !c.phase_block) return false;
    return (c.n_switches == 0 || c.switches) && (c.n_flips == 0 || c.flips);
}
}  // namespace

extern "C" int vrp_write_switchflips(const char *path, const vrp_contig *ctgs, int32_t n_ctg) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs)) return fail(VRP_ERR_ARG, "vrp_write_switchflips: bad argument");
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "CONTIG\tSTART\tSTOP\tSWITCH_TYPE\tSUPERCLUSTER\tPHASE_BLOCK\n");
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_contig &c = ctgs[ci];
        if (!phasing_ok(c)) return fail(VRP_ERR_ARG, "vrp_write_switchflips: incomplete contig");
        if (c.n_sc == 0) continue;
        // nearest supercluster with a phase of its own at or left of `k` (stops at 0) / at or right of `k` (stops at the last)
        auto phased_left = [&](int32_t k) { while (k > 0 && c.sc_phase[k] == VPR_PHASE_NONE) k--; return k; };
        auto phased_right = [&](int32_t k) { while (k < c.n_sc - 1 && c.sc_phase[k] == VPR_PHASE_NONE) k++; return k; };
        auto row = [&](int32_t from_sc, int32_t to_sc, const char *what, int32_t sc, int32_t pb) {
            fprintf(out, "%s\t%d\t%d\t%s\t%d\t%d\n", c.name, c.sc_end[from_sc], c.sc_beg[to_sc], what, sc, pb);
        };
        const bool ordered = for_each_break(c, true, true, [&](int kind, int32_t sc, int32_t pb) {
            if (kind == BRK_FLIP || kind == BRK_BLOCK_FLIP) {
                // the phasing may have changed anywhere between the last phased supercluster in front of the flipped one and
                // the flipped one, and back anywhere between it and the next phased one
                const int32_t l = phased_left(sc - 1), r = phased_right(sc + 1);
                if (l >= 0) row(l, sc, "FLIP_BEG", sc, pb);
                if (r < c.n_sc) row(sc, r, "FLIP_END", sc, pb);
            } else if (kind == BRK_SWITCH_ERR) {
                const int32_t l = phased_left(sc - 1), r = phased_right(sc);
                if (l >= 0 && r < c.n_sc) row(l, r, "SWITCH_ERR", sc, pb);
            }       // (the start of a phase block is not an error: no row)
        });
        if (!ordered) return fail(VRP_ERR_ARG, "vrp_write_switchflips: phase blocks / switches / flips are not ascending");
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}

// NG50 of the correctly phased stretches: break at phase-block starts, optionally at switch errors and around flipped
// superclusters; the genome size is the sum of the contigs' header lengths.  Returns -1 for inconsistent tables.
extern "C" int32_t vrp_ng50(const vrp_contig *ctgs, int32_t n_ctg, int32_t break_on_switch, int32_t break_on_flip) {
    if (n_ctg < 0 || (n_ctg && !ctgs)) return -1;
    uint64_t genome = 0;
    std::vector<int32_t> stretch;
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_contig &c = ctgs[ci];
        if (!phasing_ok(c)) return -1;
        genome += uint64_t(uint32_t(c.length));
        if (c.n_sc == 0) continue;
        int32_t from = c.sc_beg[0];
        auto cut = [&](int32_t last_sc, int32_t next_sc) {      // a stretch ends with last_sc, the next one starts at next_sc
            stretch.push_back(c.sc_end[last_sc] - from);
            // (a flip on the contig's last supercluster makes the reference read begs[n]: the stretch behind it is empty here)
            from = next_sc < c.n_sc ? c.sc_beg[next_sc] : c.sc_end[c.n_sc - 1];
        };
        const bool ordered = for_each_break(c, break_on_switch != 0, break_on_flip != 0, [&](int kind, int32_t sc, int32_t) {
            cut(sc - 1, sc);
            if (kind == BRK_FLIP || kind == BRK_BLOCK_FLIP) cut(sc, sc + 1);     // the flipped supercluster is a stretch of its own
        });
        if (!ordered) return -1;
        stretch.push_back(c.sc_end[c.n_sc - 1] - from);
    }
    std::sort(stretch.begin(), stretch.end(), std::greater<int32_t>());
    uint64_t covered = 0;
    for (int32_t len : stretch) {
        covered += uint64_t(int64_t(len));      // (size_t arithmetic, as in the reference)
        if (covered >= genome / 2) return len;
    }
    return 0;
}

extern "C" int vrp_write_phasing_summary(const char *path, const vrp_contig *ctgs, int32_t n_ctg) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs)) return fail(VRP_ERR_ARG, "vrp_write_phasing_summary: bad argument");
    int blocks = 0, switches = 0, flips = 0;
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        if (!phasing_ok(ctgs[ci])) return fail(VRP_ERR_ARG, "vrp_write_phasing_summary: incomplete contig");
        blocks += ctgs[ci].n_pb; switches += ctgs[ci].n_switches; flips += ctgs[ci].n_flips;
    }
    const int32_t ng50 = vrp_ng50(ctgs, n_ctg, 0, 0), sw50 = vrp_ng50(ctgs, n_ctg, 1, 0), sf50 = vrp_ng50(ctgs, n_ctg, 1, 1);
    if (ng50 < 0 || sw50 < 0 || sf50 < 0) return fail(VRP_ERR_ARG, "vrp_write_phasing_summary: phase blocks / switches / flips are not ascending");
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "PHASE_BLOCKS\tSWITCH_ERRORS\tFLIP_ERRORS\tNG_50\tSWITCH_NGC50\tSWITCHFLIP_NGC50\n");
    fprintf(out, "%d\t%d\t%d\t%d\t%d\t%d", blocks, switches, flips, ng50, sw50, sf50);      // (no newline behind the row, phase.cpp:526)
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}

extern "C" int vrp_write_superclusters(const char *path, const vrp_contig *ctgs, int32_t n_ctg) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs)) return fail(VRP_ERR_ARG, "vrp_write_superclusters: bad argument");
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "CONTIG\tSUPERCLUSTER\tSTART\tSTOP\tSIZE\tQUERY1_VARS\tQUERY2_VARS\tTRUTH1_VARS\tTRUTH2_VARS\tORIG_ED\tSWAP_ED"
                 "\tPHASE_STATE\tSC_PHASE\tPHASE_SET\tPHASE_BLOCK\tFLIP_ERROR\n");
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_contig &c = ctgs[ci];
        if (!contig_ok(c)) return fail(VRP_ERR_ARG, "vrp_write_superclusters: incomplete contig");
        if (c.n_sc > 0 && (!c.phase_block || !c.orig_phase_dist || !c.swap_phase_dist || !c.sc_phase_set))
            return fail(VRP_ERR_ARG, "vrp_write_superclusters: incomplete contig");
        int32_t pb = 0;
        for (int32_t k = 0; k < c.n_sc; k++) {
            if (k >= c.phase_block[pb + 1]) pb++;
            const int phase_switch = c.pb_phase[k] != 0, phase_sc = c.sc_phase[k];
            if (phase_sc < 0 || phase_sc > VPR_PHASE_NONE) return fail(VRP_ERR_ARG, "vrp_write_superclusters: unexpected phase");
            const int flip_error = phase_switch ? phase_sc == VPR_PHASE_ORIG : phase_sc == VPR_PHASE_SWAP;
            int32_t nv[4];
            for (int i = 0; i < 4; i++) {   // an empty hap has no cluster table at all
                const vrp_hap &h = c.hap[i];
                nv[i] = (h.n_var > 0 && c.sc_brk[i]) ? h.cluster_beg[c.sc_brk[i][k + 1]] - h.cluster_beg[c.sc_brk[i][k]] : 0;
            }
            fprintf(out, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\n", c.name, k, c.sc_beg[k], c.sc_end[k],
                    c.sc_end[k] - c.sc_beg[k], nv[0], nv[1], nv[2], nv[3], c.orig_phase_dist[k], c.swap_phase_dist[k], phase_switch,
                    PHASE_STR[phase_sc], c.sc_phase_set[k], pb, flip_error);
        }
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}

extern "C" int vrp_write_variants(const char *path, const vrp_contig *ctgs, int32_t n_ctg, int32_t callset) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs) || callset < 0 || callset > 1) return fail(VRP_ERR_ARG, "vrp_write_variants: bad argument");
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "CONTIG\tPOS\tHAP\tREF\tALT\tQUAL\tTYPE\tERRTYPE\tCREDIT\tCLUSTER\tSUPERCLUSTER\tSYNC_GROUP\tREF_DIST\tQUERY_DIST\tLOCATION\n");
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_contig &c = ctgs[ci];
        if (!contig_ok(c)) return fail(VRP_ERR_ARG, "vrp_write_variants: incomplete contig");
        const vrp_hap *H[2] = {&c.hap[2 * callset], &c.hap[2 * callset + 1]};
        int32_t v[2] = {0, 0}, cl[2] = {0, 0}, sci = 0;
        while (v[0] < H[0]->n_var || v[1] < H[1]->n_var) {
            // the two haplotypes merge by position; on equal positions the second haplotype goes first (print.cpp:692-693)
            const int h = (v[1] >= H[1]->n_var || (v[0] < H[0]->n_var && H[0]->pos[v[0]] < H[1]->pos[v[1]])) ? 0 : 1;
            const vrp_hap &V = *H[h];
            const int32_t i = v[h];
            if (cl[h] + 1 > V.n_cluster) return fail(VRP_ERR_ARG, "Out of bounds cluster during write_results()");
            if (V.cluster_beg[cl[h] + 1] <= i) cl[h]++;
            while (sci < c.n_sc && V.pos[i] >= c.sc_end[sci]) sci++;
            if (sci >= c.n_sc) return fail(VRP_ERR_ARG, "Out of bounds supercluster during write_results()");
            const int s = swap_of(c, sci);
            if (!V.errtype[s] || !V.credit[s] || !V.sync_group[s] || !V.ref_ed[s] || !V.query_ed[s] || !V.var_qual)
                return fail(VRP_ERR_ARG, "vrp_write_variants: result columns missing");
            const int et = V.errtype[s][i], ty = V.type[i], loc = V.loc ? V.loc[i] : 1;
            if (et > VPR_ERRTYPE_UN || ty > 4 || loc > 3) return fail(VRP_ERR_ARG, "vrp_write_variants: value out of range");
            fprintf(out, "%s\t%d\t%d\t%.*s\t%.*s\t%.2f\t%s\t%s\t%f\t%d\t%d\t%d\t%d\t%d\t%s\n", c.name, V.pos[i], h,
                    int(V.ref_len[i]), reinterpret_cast<const char *>(V.pool + V.ref_off[i]),
                    int(V.alt_len[i]), reinterpret_cast<const char *>(V.pool + V.alt_off[i]),
                    V.var_qual[i], TYPE_STR[ty], ERROR_STR[et], V.credit[s][i], cl[h], sci, V.sync_group[s][i],
                    V.ref_ed[s][i], V.query_ed[s][i], REGION_STR[loc]);
            v[h]++;
        }
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}

namespace {

// GA4GH-style record pieces (variant.cpp:229-286)
struct VcfOut {
    FILE *f;
    const vrp_contig *c;
    float credit_threshold;

    bool info(const vrp_hap &V, int32_t i) const {
        const char *ref = reinterpret_cast<const char *>(V.pool + V.ref_off[i]);
        const char *alt = reinterpret_cast<const char *>(V.pool + V.alt_off[i]);
        static const char FMT[] = "GT:BD:BC:RD:QD:BK:QQ:SC:SG:PS:PB:BS:FE";
        if (V.type[i] == VPR_TYPE_SUB) {
            fprintf(f, "%s\t%d\t.\t%.*s\t%.*s\t.\tPASS\t.\t%s", c->name, V.pos[i] + 1, int(V.ref_len[i]), ref, int(V.alt_len[i]), alt, FMT);
        } else if (V.type[i] == VPR_TYPE_INS || V.type[i] == VPR_TYPE_DEL) {
            if (!c->seq || V.pos[i] < 1 || V.pos[i] > c->seq_len) return false;
            const char anchor = char(c->seq[V.pos[i] - 1]);   // indels are written with the base in front of them
            fprintf(f, "%s\t%d\t.\t%c%.*s\t%c%.*s\t.\tPASS\t.\t%s", c->name, V.pos[i], anchor, int(V.ref_len[i]), ref, anchor,
                    int(V.alt_len[i]), alt, FMT);
        } else {
            return false;
        }
        return true;
    }
    void empty(int sci, int pb, bool query) const { fprintf(f, "\t.:.:.:.:.:.:.:%d:.:.:%d:.:.%s", sci, pb, query ? "\n" : ""); }
    void sample(const vrp_hap &V, int32_t i, const char *gt, int sci, int pb, bool phase_switch, bool phase_flip, bool query) const {
        const int s = phase_switch ^ phase_flip;
        const float credit = V.credit[s][i];
        const char *bd, *bk;
        if (credit == 1) { bd = "TP"; bk = "gm"; }
        else if (credit == 0) { bd = query ? "FP" : "FN"; bk = "."; }
        else if (credit >= credit_threshold) { bd = "TP"; bk = "lm"; }
        else { bd = query ? "FP" : "FN"; bk = "lm"; }
        // RD and QD are both blanked by a zero reference distance (variant.cpp:279-280)
        const bool dot = V.ref_ed[s][i] == 0;
        const std::string rd = dot ? "." : std::to_string(V.ref_ed[s][i]), qd = dot ? "." : std::to_string(V.query_ed[s][i]);
        fprintf(f, "\t%s:%s:%f:%s:%s:%s:%d:%d:%d:%d:%d:%s:%s%s", gt, bd, credit, rd.c_str(), qd.c_str(), bk, int(V.var_qual[i]), sci,
                V.sync_group[s][i], V.phase_set ? V.phase_set[i] : 0, pb, query ? (phase_switch ? "1" : "0") : ".",
                query ? (phase_flip ? "1" : "0") : ".", query ? "\n" : "");
    }
};

inline bool same_allele(const vrp_hap &A, int32_t a, const vrp_hap &B, int32_t b) {
    return A.ref_len[a] == B.ref_len[b] && A.alt_len[a] == B.alt_len[b] &&
           std::equal(A.pool + A.ref_off[a], A.pool + A.ref_off[a] + A.ref_len[a], B.pool + B.ref_off[b]) &&
           std::equal(A.pool + A.alt_off[a], A.pool + A.alt_off[a] + A.alt_len[a], B.pool + B.alt_off[b]);
}

}  // namespace

extern "C" int vrp_write_summary_vcf(const char *path, const vrp_contig *ctgs, int32_t n_ctg, const char *cmd,
                                     const char *file_date, float credit_threshold) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs)) return fail(VRP_ERR_ARG, "vrp_write_summary_vcf: bad argument");
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "##fileformat=VCFv4.2\n");
    if (file_date) {
        fprintf(out, "##fileDate=%s\n", file_date);
    } else {
        const time_t tt = time(nullptr);
        const tm lt = *localtime(&tt);
        fprintf(out, "##fileDate=%04d%02d%02d\n", lt.tm_year + 1900, lt.tm_mon + 1, lt.tm_mday);
    }
    fprintf(out, "##CL=%s\n", cmd ? cmd : "");
    for (int32_t ci = 0; ci < n_ctg; ci++)
        fprintf(out, "##contig=<ID=%s,length=%d,ploidy=%d>\n", ctgs[ci].name, ctgs[ci].length, ctgs[ci].ploidy);
    // header text of phase.cpp:24-39
    fputs("##FILTER=<ID=PASS,Description=\"All filters passed\">\n"
          "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"GenoType\">\n"
          "##FORMAT=<ID=BD,Number=1,Type=String,Description=\"Benchmark Decision for call (TP/FP/FN).\">\n"
          "##FORMAT=<ID=BC,Number=1,Type=Float,Description=\"Benchmark Credit (on the interval [0,1], based on sync group edit distance)\">\n"
          "##FORMAT=<ID=RD,Number=1,Type=Integer,Description=\"Reference edit Distance from truth within current sync group\">\n"
          "##FORMAT=<ID=QD,Number=1,Type=Integer,Description=\"Query edit Distance from truth within current sync group\">\n"
          "##FORMAT=<ID=BK,Number=1,Type=String,Description=\"BenchmarK category ('gm' if credit == 1, 'lm' if credit > 0, else '.')\">\n"
          "##FORMAT=<ID=QQ,Number=1,Type=Float,Description=\"variant Quality\">\n"
          "##FORMAT=<ID=SC,Number=1,Type=Integer,Description=\"SuperCluster (index in contig)\">\n"
          "##FORMAT=<ID=SG,Number=1,Type=Integer,Description=\"Sync Group (index in supercluster, for credit assignment)\">\n"
          "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase Set identifier (input, per-variant)\">\n"
          "##FORMAT=<ID=PB,Number=1,Type=Integer,Description=\"Phase Block (output, per-supercluster, index in contig)\">\n"
          "##FORMAT=<ID=BS,Number=1,Type=Integer,Description=\"Block State (phaseblock truth-to-query mapping state; 0 = T1Q1:T2Q2, 1 = T1Q2:T2Q1)\">\n"
          "##FORMAT=<ID=FE,Number=1,Type=Integer,Description=\"Flip Error (a per-supercluster error)\">\n"
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tTRUTH\tQUERY\n", out);

    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_contig &c = ctgs[ci];
        if (!contig_ok(c)) return fail(VRP_ERR_ARG, "vrp_write_summary_vcf: incomplete contig");
        if (c.n_sc == 0) continue;
        if (!c.phase_block) return fail(VRP_ERR_ARG, "vrp_write_summary_vcf: incomplete contig");
        const VcfOut w{out, &c, credit_threshold};
        const vrp_hap *Q[2] = {&c.hap[0], &c.hap[1]}, *T[2] = {&c.hap[2], &c.hap[3]};
        for (int i = 0; i < 4; i++)
            if (c.hap[i].n_var > 0 && (!c.hap[i].credit[0] || !c.hap[i].credit[1] || !c.hap[i].ref_ed[0] || !c.hap[i].ref_ed[1] ||
                                       !c.hap[i].query_ed[0] || !c.hap[i].query_ed[1] || !c.hap[i].sync_group[0] ||
                                       !c.hap[i].sync_group[1] || !c.hap[i].var_qual))
                return fail(VRP_ERR_ARG, "vrp_write_summary_vcf: result columns missing");
        int32_t ptr[4] = {0, 0, 0, 0};
        int32_t sci = 0, pb = 0;
        bool phase_switch = false, phase_flip = false;
        int swap = 0;
        // a supercluster whose own phase contradicts its block's state is a flip error and keeps its own evaluation
        auto enter = [&](int32_t k) {
            phase_switch = c.pb_phase[k] != 0;
            const int psc = c.sc_phase[k];
            phase_flip = phase_switch ? psc == VPR_PHASE_ORIG : psc == VPR_PHASE_SWAP;
            swap = int(phase_switch) ^ int(phase_flip);
        };
        enter(0);
        auto left = [&]() { for (int i = 0; i < 4; i++) if (ptr[i] < c.hap[i].n_var) return true; return false; };
        const bool haploid = c.ploidy == 1;
        while (left()) {
            // next record position: indels are keyed by their anchor base
            int32_t at[4];
            for (int i = 0; i < 4; i++) {
                const vrp_hap &V = c.hap[i];
                at[i] = INT_MAX;
                if (ptr[i] < V.n_var) at[i] = V.pos[ptr[i]] - (V.type[ptr[i]] == VPR_TYPE_INS || V.type[ptr[i]] == VPR_TYPE_DEL);
            }
            const int32_t pos = std::min(std::min(at[0], at[1]), std::min(at[2], at[3]));
            bool nq[2] = {at[0] == pos, at[1] == pos}, nt[2] = {at[2] == pos, at[3] == pos};
            if (pos >= c.sc_end[sci]) {   // one step at most, as in the reference (phase.cpp:104)
                if (++sci >= c.n_sc) return fail(VRP_ERR_ARG, "vrp_write_summary_vcf: variant behind the last supercluster");
                if (sci >= c.phase_block[pb + 1]) pb++;
                enter(sci);
            }
            bool pair[2];
            for (int h = 0; h < 2; h++)
                pair[h] = nq[h] && nt[swap ^ h] && same_allele(*Q[h], ptr[h], *T[swap ^ h], ptr[2 + (swap ^ h)]);
            auto gt_of = [&](int hap) { return haploid ? "1" : hap ? "0|1" : "1|0"; };
            auto emit_query = [&](int h, const char *gq, const char *gtr) {   // one record led by query hap h
                const int th = h ^ swap;
                if (!w.info(*Q[h], ptr[h])) return false;
                if (pair[h]) { w.sample(*T[th], ptr[2 + th], gtr, sci, pb, phase_switch, phase_flip, false); }
                else w.empty(sci, pb, false);
                w.sample(*Q[h], ptr[h], gq, sci, pb, phase_switch, phase_flip, true);
                ptr[h]++;
                if (pair[h]) ptr[2 + th]++;
                return true;
            };
            auto emit_truth = [&](int h, const char *gtr) {   // truth-only record on the truth hap paired with query hap h
                const int th = h ^ swap;
                if (!w.info(*T[th], ptr[2 + th])) return false;
                w.sample(*T[th], ptr[2 + th], gtr, sci, pb, phase_switch, phase_flip, false);
                w.empty(sci, pb, true);
                ptr[2 + th]++;
                return true;
            };
            bool ok = true;
            if (nq[0] && nq[1]) {          // homozygous-looking pairs stay two records (their credit may differ)
                for (int h = 0; h < 2 && ok; h++) ok = emit_query(h, h ? "0|1" : "1|0", (h ^ swap) ? "0|1" : "1|0");
            } else if (nq[0]) {
                ok = emit_query(0, gt_of(0), gt_of(0 ^ swap));
            } else if (nq[1]) {
                ok = emit_query(1, gt_of(1), gt_of(1 ^ swap));
            } else if (nt[0] && nt[1]) {
                for (int h = 0; h < 2 && ok; h++) ok = emit_truth(h, (h ^ swap) ? "0|1" : "1|0");
            } else if (nt[0 ^ swap]) {
                ok = emit_truth(0, gt_of(0 ^ swap));
            } else if (nt[1 ^ swap]) {
                ok = emit_truth(1, gt_of(1 ^ swap));
            } else {
                return fail(VRP_ERR_ARG, "No variants are selected next.");
            }
            if (!ok) return fail(VRP_ERR_ARG, "vrp_write_summary_vcf: variant type / anchor base unavailable");
        }
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The distance files (editData::write_distance / write_edits, src/edit.cpp:134-280).  The reference rescans every edit for every
// quality and type (get_ed / get_de / get_score, edit.cpp:105-132); the counters here come from difference arrays over the
// records' [min_qual, max_qual) ranges, one pass over the records: the same integers.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

const char *const TYPE_STR2[] = {"ALL", "SNP", "INS", "DEL", "INDEL"};

bool in_category(int type, int cat) { return cat == 0 || type == cat || (cat == 4 && (type == VPR_TYPE_INS || type == VPR_TYPE_DEL)); }
float dist_qscore(double p) { return float(std::min(100.0, std::max(0.0, -10 * std::log10(p)))); }

struct DistCounters {
    int32_t q0 = 0, n = 0;                    // qualities q0 .. q0 + n - 1
    std::vector<int64_t> ed[5], de[5], score;
    int32_t ED(int q, int c) const { return int32_t(ed[c][size_t(q - q0)]); }
    int32_t DE(int q, int c) const { return int32_t(de[c][size_t(q - q0)]); }
    int32_t SC(int q) const { return int32_t(score[size_t(q - q0)]); }
};

bool dist_counters(const vrp_edits *sets, int32_t n_sets, int32_t min_qual, int32_t max_qual, int32_t sub, int32_t open, int32_t extend,
                   DistCounters &C) {
    C.q0 = std::min(min_qual, 0);
    const int32_t q1 = max_qual + 2;          // queries run over [min_qual, max_qual + 1]
    C.n = q1 - C.q0;
    for (int c = 0; c < 5; c++) { C.ed[c].assign(size_t(C.n) + 1, 0); C.de[c].assign(size_t(C.n) + 1, 0); }
    C.score.assign(size_t(C.n) + 1, 0);
    for (int32_t k = 0; k < n_sets; k++) {
        const vrp_edits &E = sets[k];
        if (E.n > 0 && (!E.type || !E.len || !E.min_qual || !E.max_qual)) return false;
        for (int64_t i = 0; i < E.n; i++) {
            const int lo = std::max(E.min_qual[i], C.q0), hi = std::min(E.max_qual[i], q1);
            if (lo >= hi) continue;
            const size_t a = size_t(lo - C.q0), b = size_t(hi - C.q0);
            const int type = E.type[i];
            for (int c = 0; c < 5; c++)
                if (in_category(type, c)) { C.ed[c][a] += E.len[i]; C.ed[c][b] -= E.len[i]; C.de[c][a]++; C.de[c][b]--; }
            const int64_t w = type == VPR_TYPE_SUB ? sub : (type == VPR_TYPE_INS || type == VPR_TYPE_DEL) ? int64_t(open) + int64_t(extend) * E.len[i] : 0;
            C.score[a] += w; C.score[b] -= w;
        }
    }
    auto run = [&](std::vector<int64_t> &v) { for (size_t i = 1; i < v.size(); i++) v[i] += v[i - 1]; };
    for (int c = 0; c < 5; c++) { run(C.ed[c]); run(C.de[c]); }
    run(C.score);
    return true;
}

}  // namespace

extern "C" int vrp_write_distance(const char *prefix, const vrp_edits *sets, int32_t n_sets, int32_t min_qual, int32_t max_qual,
                                  int32_t eval_sub, int32_t eval_open, int32_t eval_extend, int32_t verbosity, int32_t write_files,
                                  char *summary, int64_t summary_cap) {
    if ((n_sets && !sets) || n_sets < 0 || max_qual + 1 < min_qual || (write_files && !prefix)) return fail(VRP_ERR_ARG, "vrp_write_distance: bad arguments");
    DistCounters C;
    if (!dist_counters(sets, n_sets, min_qual, max_qual, eval_sub, eval_open, eval_extend, C)) return fail(VRP_ERR_ARG, "vrp_write_distance: null column");
    const std::string pre = prefix ? prefix : "";
    const int top = max_qual + 1;
    const int orig = C.SC(top);
    int orig_ed[5], orig_de[5], best_q[5];
    double best[5];
    for (int c = 0; c < 5; c++) { orig_ed[c] = C.ED(top, c); orig_de[c] = C.DE(top, c); best[c] = std::numeric_limits<double>::max(); best_q[c] = 0; }
    {
        File f(write_files ? (pre + "distance.tsv").c_str() : nullptr);
        if (write_files && !f) return fail(VRP_ERR_OPEN, "cannot create " + pre + "distance.tsv");
        if (f) fprintf(f, "MIN_QUAL\tSUB_DE\tINS_DE\tDEL_DE\tSUB_ED\tINS_ED\tDEL_ED\tDISTINCT_EDITS\tEDIT_DIST\tALN_SCORE\tALN_QSCORE\n");
        for (int q = min_qual; q <= top; q++) {
            for (int c = 0; c < 5; c++) {
                const double v = double(C.ED(q, c)) * C.DE(q, c);
                if (v < best[c]) { best[c] = v; best_q[c] = q; }
            }
            if (f) fprintf(f, "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%f\n", q, C.DE(q, 1), C.DE(q, 2), C.DE(q, 3), C.ED(q, 1), C.ED(q, 2),
                           C.ED(q, 3), C.DE(q, 0), C.ED(q, 0), C.SC(q), dist_qscore(double(C.SC(q)) / orig));
        }
        if (f && !f.finish()) return fail(VRP_ERR_OPEN, "write to " + pre + "distance.tsv failed");
    }
    std::string txt = "ALIGNMENT DISTANCE SUMMARY\n";
    {
        File g(write_files ? (pre + "distance-summary.tsv").c_str() : nullptr);
        if (write_files && !g) return fail(VRP_ERR_OPEN, "cannot create " + pre + "distance-summary.tsv");
        if (g) fprintf(g, "VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE\n");
        char line[512];
        for (int c = 0; c < 5; c++) {
            // the reference's verbosity filter (edit.cpp:212-217) skips a type before anything is written: stdout and file alike
            if ((verbosity == 0 && c != 0) || (verbosity == 1 && (c == VPR_TYPE_INS || c == VPR_TYPE_DEL))) continue;
            txt += c == 0 ? "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE\n"
                          : "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\n";
            const int qs[3] = {min_qual, best_q[c], top};
            const char *const names[3] = {"NONE", "BEST", "REF "};
            for (int i = 0; i < 3; i++) {
                const int q = qs[i];
                const float eq = dist_qscore(double(C.ED(q, c)) / orig_ed[c]), dq = dist_qscore(double(C.DE(q, c)) / orig_de[c]);
                const float aq = c == 0 ? dist_qscore(double(C.SC(q)) / orig) : 0;
                if (g) fprintf(g, "%s\t%s\t%d\t%d\t%d\t%f\t%f\t%f\n", TYPE_STR2[c], names[i], q, C.ED(q, c), C.DE(q, c), eq, dq, aq);
                if (c == 0) snprintf(line, sizeof(line), "%s\t%s Q >= %d\t%-16d%-16d%f\t%f\t%f\n", TYPE_STR2[c], names[i], q, C.ED(q, c), C.DE(q, c), eq, dq, aq);
                else snprintf(line, sizeof(line), "%s\t%s Q >= %d\t%-16d%-16d%f\t%f\n", TYPE_STR2[c], names[i], q, C.ED(q, c), C.DE(q, c), eq, dq);
                txt += line;
            }
        }
        if (g && !g.finish()) return fail(VRP_ERR_OPEN, "write to " + pre + "distance-summary.tsv failed");
    }
    if (summary && summary_cap > 0) snprintf(summary, size_t(summary_cap), "%s", txt.c_str());
    return int(txt.size());
}

extern "C" int vrp_write_edits(const char *path, const vrp_edits *sets, int32_t n_sets) {
    if (!path || (n_sets && !sets) || n_sets < 0) return fail(VRP_ERR_ARG, "vrp_write_edits: bad arguments");
    File f(path);
    if (!f) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(f, "CONTIG\tSTART\tHAP\tTYPE\tSIZE\tSUPERCLUSTER\tMIN_QUAL\tMAX_QUAL\n");
    for (int32_t k = 0; k < n_sets; k++) {
        const vrp_edits &E = sets[k];
        for (int64_t i = 0; i < E.n; i++) {
            const int type = E.type[i];
            if (type < 0 || type > 4) return fail(VRP_ERR_ARG, "vrp_write_edits: bad edit type");
            fprintf(f, "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n", E.ctg, E.pos[i], int(E.hap[i]), TYPE_STR[type], E.len[i], E.sc[i], E.min_qual[i],
                    E.max_qual[i]);
        }
    }
    if (!f.finish()) return fail(VRP_ERR_OPEN, std::string("write to ") + path + " failed");
    return VRP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// A callset as a VCF (variantData::write_vcf + print_variant, src/variant.cpp:132-222, 292-315): orig-query.vcf, query.vcf ... of
// the realignment modes.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int vrp_write_vcf(const char *path, const vrp_vcf_contig *ctgs, int32_t n_ctg, const char *sample, const char *file_date) {
    if (!path || n_ctg < 0 || (n_ctg && !ctgs)) return fail(VRP_ERR_ARG, "vrp_write_vcf: bad argument");
    for (int32_t ci = 0; ci < n_ctg; ci++)
        for (int h = 0; h < 2; h++) {
            const vrp_hap &H = ctgs[ci].hap[h];
            if (H.n_var < 0 || (H.n_var && (!H.pos || !H.type || !H.var_qual || !H.ref_len || !H.alt_len || !H.ref_off || !H.alt_off || !H.pool)))
                return fail(VRP_ERR_ARG, "vrp_write_vcf: incomplete variant columns");
        }
    File out(path);
    if (!out) return fail(VRP_ERR_OPEN, std::string("cannot create ") + path);
    fprintf(out, "##fileformat=VCFv4.2\n");
    if (file_date) {
        fprintf(out, "##fileDate=%s\n", file_date);
    } else {
        const time_t tt = time(nullptr);
        const tm lt = *localtime(&tt);
        fprintf(out, "##fileDate=%04d%02d%02d\n", lt.tm_year + 1900, lt.tm_mon + 1, lt.tm_mday);
    }
    for (int32_t ci = 0; ci < n_ctg; ci++)
        fprintf(out, "##contig=<ID=%s,length=%d,ploidy=%d>\n", ctgs[ci].name, ctgs[ci].length, ctgs[ci].ploidy);
    fprintf(out, "##FILTER=<ID=PASS,Description=\"All filters passed\">\n");
    fprintf(out, "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n");
    fprintf(out, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", sample ? sample : "");
    std::string ref, alt;
    for (int32_t ci = 0; ci < n_ctg; ci++) {
        const vrp_vcf_contig &c = ctgs[ci];
        // print_variant: an INS / DEL at pos (already one left) gets the anchor base in front of both alleles
        auto print = [&](const vrp_hap &H, int32_t i, int pos, const char *gt) {
            const int type = H.type[i];
            ref.assign(reinterpret_cast<const char *>(H.pool + H.ref_off[i]), size_t(H.ref_len[i]));
            alt.assign(reinterpret_cast<const char *>(H.pool + H.alt_off[i]), size_t(H.alt_len[i]));
            if (type == VPR_TYPE_INS || type == VPR_TYPE_DEL) {
                if (!c.seq || pos < 0 || pos >= c.seq_len) return false;
                const char base = char(c.seq[pos]);
                ref.insert(ref.begin(), base);
                alt.insert(alt.begin(), base);
            } else if (type != VPR_TYPE_SUB) {
                return false;
            }
            fprintf(out, "%s\t%d\t.\t%s\t%s\t%f\tPASS\t.\tGT\t%s\n", c.name, pos + 1, ref.c_str(), alt.c_str(), H.var_qual[i], gt);
            return true;
        };
        const vrp_hap &A = c.hap[0], &B = c.hap[1];
        int32_t pa = 0, pb = 0;
        while (pa < A.n_var || pb < B.n_var) {
            auto at = [](const vrp_hap &H, int32_t p) {
                if (p >= H.n_var) return INT32_MAX;
                return H.type[p] == VPR_TYPE_INS || H.type[p] == VPR_TYPE_DEL ? H.pos[p] - 1 : H.pos[p];
            };
            const int p1 = at(A, pa), p2 = at(B, pb), pos = std::min(p1, p2);
            const bool h1 = p1 == pos, h2 = p2 == pos;
            bool ok = true;
            if (h1 && h2) {
                if (same_allele(A, pa, B, pb)) ok = print(A, pa, pos, "1|1");
                else ok = print(A, pa, pos, "1|0") && print(B, pb, pos, "0|1");
            } else if (h1) {
                ok = print(A, pa, pos, c.ploidy == 1 ? "1" : "1|0");
            } else {
                ok = print(B, pb, pos, c.ploidy == 1 ? "1" : "0|1");
            }
            if (!ok) return fail(VRP_ERR_ARG, std::string("vrp_write_vcf: variant type / anchor base unavailable on ") + c.name);
            if (h1) pa++;
            if (h2) pb++;
        }
    }
    if (!out.finish()) return fail(VRP_ERR_OPEN, std::string("write error on ") + path);
    return VRP_OK;
}
