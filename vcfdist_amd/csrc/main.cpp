// main.cpp -- vcfdist_gpu: the reference's command line for the precision/recall evaluation with the host orchestration in C++
// (main.cpp / globals.cpp of vcfdist v2.6.4: parse the arguments, read the VCFs / BED / FASTA, per contig cluster -> supercluster
// -> precision_recall_wrapper -> phase, then the counters, the PRECISION-RECALL SUMMARY and the output files) over the C ABIs of
// this repository: include/vcfdist_io.h (readers), vcfdist_cluster.h (clustering on the GPU / host, superclustering),
// vcfdist_pr.h (the alignment path on the GPU: generate_ptrs_strs on the device, vpr_execute, phasing, counters),
// vcfdist_report.h (writers).  One process, one GPU; the sharded runs (one process per GPU, RCCL) are `python -m vcfdist_amd`
// under torch.distributed.run, which is the same sequence of calls.  No CPU fallback: without a HIP device vpr_create fails.
//
// The stages carry the names of the Python driver's (vcfdist_amd/__main__.py): main() parses, reads (read_inputs), plans the strata
// (plan_strata), realigns (realign_inputs), runs the k-mer passes, then per contig prepare_contig and evaluate_contig -- which owns
// the order of the library calls --, then write_outputs and report.  Inputs, StrataPlan and Totals hold what lives across contigs.
//
//   vcfdist_gpu <query.vcf[.gz]> <truth.vcf[.gz]> <ref.fasta[.gz]> [-b regions.bed] [-p prefix] [-n] [-c biwfa | gap N | size N] [-l max variant size]
//               [-s max supercluster size] [-mn / -mx qual] [-f filters] [-i iterations] [-x -o -e penalties] [-ct credit threshold] [-pt phasing threshold]
//               [-sv threshold] [--reach-min-gap N] [--strict] [--device N] [-d] [-ex -eo -ee evaluation penalties] [-rq] [-rt] [-ro] [--stratify strata.tsv]
//               [--stratify-repeats] [--stratify-long-repeats] [--stratify-near-repeats K:M[,K:M...]] [--stratify-context] [--stratify-variants] [--stratify-derive NAME=EXPR]... [--stratify-cross LIST:LIST]... [--bootstrap N] [--bootstrap-seed S]
//               [--classify-errors] [--error-window N] [--classify-matches] [--cut-classes]
// What an option adds (its header under include/ says how) and the files it writes:
//   -d                       vcfdist_distance.h: the distance metrics (edits_wrapper, dist.cpp:1908-2077) behind each contig's path (main.cpp:223-238)
//   -rq / -rt / -ro          vcfdist_realign.h: a callset clustered and realigned before the evaluation (main.cpp:50-180): orig-*.vcf, query.vcf /
//                            truth.vcf; -ro stops there
//   --stratify FILE          vcfdist_strata.h: the counters also cut by the BEDs of a GIAB list (name<TAB>path): stratified-precision-recall[-summary].tsv
//   --stratify-repeats       vcfdist_repeats.h: default strata where the FASTA is not unique, one genome-wide pass before the contigs: repeat-strata.bed
//   --stratify-long-repeats  vcfdist_longrepeats.h: repeated 64-, 100- and 250-mers, one more genome-wide pass: long-repeat-strata.bed
//   --stratify-near-repeats  vcfdist_nearrepeats.h: K-mers that occur again within M substitutions (the user's entries, near_k<K>_m<M>), one
//                            more genome-wide pass: near-repeat-strata.bed
//   --stratify-context       vcfdist_context.h: homopolymers, short tandem repeats, GC bands, intervals built from the FASTA: context-strata.bed
//   --stratify-variants      vcfdist_varstrata.h: transitions / transversions, indel size bins, hom / het, isolated / crowded: variant-strata.tsv
//                            (the strata stand in this order in every table; each default set also stands alone)
//   --stratify-derive        vcfdist_derive.h: NAME=EXPR, a stratum made from the membership bits of the strata in front of it (& | ! and parentheses
//                            over names, '*' globs for the union of what they match), repeatable, behind every other stratum: derived-strata.tsv
//   --stratify-cross         vcfdist_derive.h: LIST:LIST, the strata a&b of every pair of two lists of globs, repeatable, behind the derived ones
//                            (both need another --stratify* option; at most VPR_DV_MAX_CLI of them in all)
//   --classify-errors        vcfdist_errclass.h: the first error class that applies to every query FP and truth FN, something within --error-window N
//                            bases (default 50) among them: error-classes[-summary].tsv
//   --classify-matches       vcfdist_matchkind.h: exact, shifted, regrouped or partial for every TP of either callset: match-kinds[-summary].tsv
//   --cut-classes            vcfdist_labelcut.h: the label counts of every active pass cut by the strata and resampled as well: stratified-error-classes
//                            [-summary].tsv, bootstrap-error-classes-summary.tsv and their match-kinds counterparts; without it no file changes
//   --bootstrap N            vcfdist_bootstrap.h: a Poisson bootstrap over superclusters, conditional on the phasing: bootstrap-precision-recall-summary.tsv
//                            (95 % percentile intervals), bootstrap-replicates.tsv, with strata stratified-bootstrap-precision-recall-summary.tsv
#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/vcfdist_bootstrap.h"
#include "../../include/vcfdist_cluster.h"
#include "../../include/vcfdist_distance.h"
#include "../../include/vcfdist_io.h"
#include "../../include/vcfdist_pr.h"
#include "../../include/vcfdist_realign.h"
#include "../../include/vcfdist_report.h"
#include "../../include/vcfdist_context.h"
#include "../../include/vcfdist_repeats.h"
#include "../../include/vcfdist_longrepeats.h"
#include "../../include/vcfdist_nearrepeats.h"
#include "../../include/vcfdist_strata.h"
#include "../../include/vcfdist_varstrata.h"
#include "../../include/vcfdist_derive.h"
#include "../../include/vcfdist_errclass.h"
#include "../../include/vcfdist_matchkind.h"

namespace {

struct Args {
    std::string query, truth, fasta, bed, filter, prefix = "./", cluster = "biwfa", stratify;
    bool stratify_context = false, stratify_variants = false, stratify_repeats = false, stratify_long_repeats = false;
    std::vector<vpr_near_stratum> near;    // --stratify-near-repeats: the entries (empty: not given)
    std::vector<std::string> derive, cross;     // --stratify-derive, --stratify-cross: the entries as given, in command-line order
    int max_size = 5000, min_qual = 0, max_qual = 60, cluster_gap = 50, max_iterations = 4, max_supercluster_size = 10000;
    int sub = 5, open = 6, extend = 2, sv_threshold = 50, reach_min_gap = 10, device = 0;
    int eval_sub = 3, eval_open = 2, eval_extend = 1;      // globals.h:52-55
    bool distance = false;
    bool realign_query = false, realign_truth = false, realign_only = false;
    double credit_threshold = 0.7, phase_threshold = 0.6;
    bool no_output_files = false, strict = false;
    int bootstrap = 0;                 // --bootstrap: replicates (0: none)
    bool classify_errors = false;      // --classify-errors
    int error_window = -1;             // --error-window: -1 not given (VPR_EC_DEFAULT_WINDOW)
    bool classify_matches = false;     // --classify-matches
    bool cut_classes = false;          // --cut-classes
    uint64_t bootstrap_seed = 1;
};

[[noreturn]] void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    exit(1);
}
// an evaluation penalty as globals.cpp:274-335 reads it: std::stoi, then non-negative
int eval_penalty(const char *v, const char *what) {
    int x = 0;
    try { x = std::stoi(v); } catch (const std::exception &) { die("ERROR: Invalid %s provided", what); }
    if (x < 0) die("ERROR: Must provide non-negative %s", what);
    return x;
}
// --bootstrap N: 1 to VPR_BOOT_MAX_REPLICATES; --bootstrap-seed S: an unsigned 64-bit integer
int bootstrap_replicates(const char *v) {
    char *end = nullptr;
    errno = 0;
    const long long n = strtoll(v, &end, 10);
    if (end == v || *end || errno) die("ERROR: Invalid number of bootstrap replicates '%s'", v);
    if (n < 1 || n > VPR_BOOT_MAX_REPLICATES) die("ERROR: Must provide 1 to %d bootstrap replicates", VPR_BOOT_MAX_REPLICATES);
    return int(n);
}
uint64_t bootstrap_seed(const char *v) {
    char *end = nullptr;
    errno = 0;
    const unsigned long long s = strtoull(v, &end, 10);
    if (end == v || *end || errno || v[0] == '-') die("ERROR: Invalid bootstrap seed '%s'", v);
    return s;
}
// --error-window N: a non-negative 32-bit integer
int error_window(const char *v) {
    char *end = nullptr;
    errno = 0;
    const long long n = strtoll(v, &end, 10);
    if (end == v || *end || errno) die("ERROR: Invalid error window '%s'", v);
    if (n < 0 || n > INT32_MAX) die("ERROR: Must provide an error window of 0 to %d bases", INT32_MAX);
    return int(n);
}
// --stratify-near-repeats K:M[,K:M...]: numbers within the limits of include/vcfdist_nearrepeats.h, no entry twice, at most four
std::vector<vpr_near_stratum> near_strata(const std::string &text) {
    static const char *O = "--stratify-near-repeats";
    std::vector<vpr_near_stratum> specs;
    auto number = [](const std::string &t, int &x) {
        if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos) return false;
        x = atoi(t.c_str());
        return true;
    };
    size_t at = 0;
    while (true) {
        const size_t comma = text.find(',', at);
        const std::string entry = text.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        const size_t colon = entry.find(':');
        int k = 0, m = 0;
        if (colon == std::string::npos || !number(entry.substr(0, colon), k) || !number(entry.substr(colon + 1), m))
            die("ERROR: %s: entry '%s' is not K:M", O, entry.c_str());
        if (m > VPR_NREP_MAX_M || k < 8 * (m + 1) || k > VPR_NREP_MAX_K)
            die("ERROR: %s: entry '%s': M must be 0 to %d and K 8 (M + 1) to %d", O, entry.c_str(), VPR_NREP_MAX_M, VPR_NREP_MAX_K);
        for (const vpr_near_stratum &sp : specs)
            if (sp.k == k && sp.m == m) die("ERROR: %s: duplicate entry '%s'", O, entry.c_str());
        if (specs.size() == VPR_NREP_MAX_SPEC) die("ERROR: %s: more than %d entries", O, VPR_NREP_MAX_SPEC);
        specs.push_back(vpr_near_stratum{k, m, 0});
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    return specs;
}
void warn(const std::string &m) { fprintf(stderr, "[WARN  vcfdist] %s\n", m.c_str()); }

Args parse(int argc, char **argv) {
    Args a;
    std::vector<std::string> pos;
    auto need = [&](int &i) -> const char * { if (i + 1 >= argc) die("ERROR: option '%s' needs a value", argv[i]); return argv[++i]; };
    for (int i = 1; i < argc; i++) {
        const std::string o = argv[i];
        if (o == "-b" || o == "--bed") a.bed = need(i);
        else if (o == "-f" || o == "--filter") a.filter = need(i);
        else if (o == "-l" || o == "--largest-variant") a.max_size = atoi(need(i));
        else if (o == "-mn" || o == "--min-qual") a.min_qual = atoi(need(i));
        else if (o == "-mx" || o == "--max-qual") a.max_qual = atoi(need(i));
        else if (o == "-c" || o == "--cluster") {
            a.cluster = need(i);
            if ((a.cluster == "gap" || a.cluster == "size") && i + 1 < argc && argv[i + 1][0] != '-') a.cluster_gap = atoi(argv[++i]);
            if (a.cluster != "biwfa" && a.cluster != "gap" && a.cluster != "size") die("ERROR: unknown clustering method '%s'", a.cluster.c_str());
        }
        else if (o == "-i" || o == "--max-iterations") a.max_iterations = atoi(need(i));
        else if (o == "-s" || o == "--max-supercluster-size") a.max_supercluster_size = atoi(need(i));
        else if (o == "-x" || o == "--mismatch-penalty") a.sub = atoi(need(i));
        else if (o == "-o" || o == "--gap-open-penalty") a.open = atoi(need(i));
        else if (o == "-e" || o == "--gap-extend-penalty") a.extend = atoi(need(i));
        else if (o == "-ct" || o == "--credit-threshold") a.credit_threshold = atof(need(i));
        else if (o == "-pt" || o == "--phasing-threshold") a.phase_threshold = atof(need(i));
        else if (o == "-sv" || o == "--sv-threshold") a.sv_threshold = atoi(need(i));
        else if (o == "--reach-min-gap") a.reach_min_gap = atoi(need(i));
        else if (o == "-p" || o == "--prefix") a.prefix = need(i);
        else if (o == "-n" || o == "--no-output-files") a.no_output_files = true;
        else if (o == "--strict") a.strict = true;
        else if (o == "--device") a.device = atoi(need(i));
        else if (o == "-d" || o == "--distance") a.distance = true;
        else if (o == "--stratify") a.stratify = need(i);
        else if (o == "--stratify-context") a.stratify_context = true;
        else if (o == "--stratify-repeats") a.stratify_repeats = true;
        else if (o == "--stratify-long-repeats") a.stratify_long_repeats = true;
        else if (o == "--stratify-near-repeats") a.near = near_strata(need(i));
        else if (o == "--stratify-variants") a.stratify_variants = true;
        else if (o == "--stratify-derive") a.derive.push_back(need(i));
        else if (o == "--stratify-cross") a.cross.push_back(need(i));
        else if (o == "--bootstrap") a.bootstrap = bootstrap_replicates(need(i));
        else if (o == "--bootstrap-seed") a.bootstrap_seed = bootstrap_seed(need(i));
        else if (o == "--classify-errors") a.classify_errors = true;
        else if (o == "--error-window") a.error_window = error_window(need(i));
        else if (o == "--classify-matches") a.classify_matches = true;
        else if (o == "--cut-classes") a.cut_classes = true;
        else if (o == "-rq" || o == "--realign-query") a.realign_query = true;
        else if (o == "-rt" || o == "--realign-truth") a.realign_truth = true;
        else if (o == "-ro" || o == "--realign-only") a.realign_only = true;
        else if (o == "-ex" || o == "--eval-mismatch-penalty") a.eval_sub = eval_penalty(need(i), "evaluation mismatch penalty");
        else if (o == "-eo" || o == "--eval-gap-open-penalty") a.eval_open = eval_penalty(need(i), "eval gap-opening penalty");
        else if (o == "-ee" || o == "--eval-gap-extend-penalty") a.eval_extend = eval_penalty(need(i), "eval gap-extension penalty");
        else if (!o.empty() && o[0] == '-' && o.size() > 1) die("ERROR: unknown option '%s'", o.c_str());
        else pos.push_back(o);
    }
    if (pos.size() != 3) die("usage: vcfdist_gpu <query.vcf> <truth.vcf> <ref.fasta> [options]");
    a.query = pos[0]; a.truth = pos[1]; a.fasta = pos[2];
    if (a.max_size + 2 > a.max_supercluster_size)          // globals.cpp:478-481
        die("ERROR: Max supercluster size (-s) must be at least two larger than max variant size (-l).");
    if (a.error_window >= 0 && !a.classify_errors) die("ERROR: --error-window needs --classify-errors");
    if (a.error_window < 0) a.error_window = VPR_EC_DEFAULT_WINDOW;
    if (a.cut_classes && !a.classify_errors && !a.classify_matches) die("ERROR: --cut-classes needs --classify-errors or --classify-matches");
    if (a.cut_classes && a.stratify.empty() && !a.stratify_repeats && !a.stratify_long_repeats && a.near.empty() && !a.stratify_context && !a.stratify_variants && !a.bootstrap)
        die("ERROR: --cut-classes needs --stratify, --stratify-context, --stratify-variants or --bootstrap");
    if ((a.realign_query || a.realign_truth) && (a.sub < 1 || a.extend < 1))
        die("ERROR: realignment needs a mismatch penalty (-x) and a gap-extension penalty (-e) of at least 1");
    return a;
}

int find(const std::vector<std::string> &v, const std::string &s) {
    for (size_t i = 0; i < v.size(); i++) if (v[i] == s) return int(i);
    return -1;
}
void add_into(int64_t *a, const int64_t *b, size_t n) { for (size_t k = 0; k < n; k++) a[k] += b[k]; }
void wrote(int rc) { if (rc) die("ERROR: %s", vrp_last_error()); }       // every writer of include/vcfdist_report.h goes through here
std::vector<const char *> c_strs(const std::vector<std::string> &v) {
    std::vector<const char *> p;
    for (const auto &s : v) p.push_back(s.c_str());
    return p;
}
struct Pinned { Pinned() = default; Pinned(const Pinned &) = delete; Pinned &operator=(const Pinned &) = delete; };     // (others point into it)

// ---- the views of a hap's columns (vio_hap_vars) that the clustering and the writers take
const vio_hap_vars EMPTY_HAP = {0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
const uint8_t NO_POOL[1] = {0};          // (the allele pool of a hap without alleles: a pointer is wanted)
const uint8_t *pool_of(const vio_hap_vars &s) { return s.pool ? s.pool : NO_POOL; }
vcl_hap hap_cols(const vio_hap_vars &s) { return vcl_hap{s.n, s.pos, s.rlen, s.type, s.ref_len, s.alt_len}; }
vcl_hap_seq hap_seq(const vio_hap_vars &s) { return vcl_hap_seq{hap_cols(s), s.ref_off, s.alt_off, pool_of(s)}; }
// the columns a writer reads of every hap (the caller has zeroed the rest)
void hap_view(vrp_hap &hp, const vio_hap_vars &v) {
    hp.n_var = v.n; hp.pos = v.pos; hp.type = v.type; hp.var_qual = v.var_qual; hp.ref_len = v.ref_len; hp.alt_len = v.alt_len;
    hp.ref_off = v.ref_off; hp.alt_off = v.alt_off; hp.pool = pool_of(v);
}

// ---- what was read: the -b BED, both callsets, the FASTA, and the realigned columns that stand in for a callset's own
struct Inputs : Pinned {
    vio_bed *bed = nullptr;
    vio_callset *q = nullptr, *t = nullptr;
    vio_fasta *fa = nullptr;
    std::vector<std::string> bedc, qn, tn, fn;           // contig names of the BED (in the order it first names them), the VCFs, the FASTA
    vio_hap_vars *q_read = nullptr, *t_read = nullptr;   // the callsets' columns as read (realign_callset points vars elsewhere)
    std::vector<vrl_result *> realigned;
    std::vector<vio_hap_vars> q_cols, t_cols;
    ~Inputs() {
        for (vrl_result *r : realigned) vrl_result_free(r);
        if (q) { q->vars = q_read; vio_callset_free(q); }
        if (t) { t->vars = t_read; vio_callset_free(t); }
        if (fa) vio_fasta_free(fa);
        if (bed) vio_bed_free(bed);
    }
    const uint8_t *seq(int fi) const { return fa->seq + fa->ctg_off[fi]; }                   // a contig of the FASTA
    int64_t seq_len(int fi) const { return fa->ctg_off[fi + 1] - fa->ctg_off[fi]; }
};
// contigs of a BED file in the order it first names them (bedData::contigs, bed.cpp:22-26)
std::vector<std::string> bed_contigs(const std::string &path) {
    std::vector<std::string> out;
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string c;
        if (ss >> c && std::find(out.begin(), out.end(), c) == out.end()) out.push_back(c);
    }
    return out;
}
// both callsets inside the -b BED (main has read it), the FASTA, and the contig names of all four
void read_inputs(const Args &A, Inputs &in) {
    if (in.bed) in.bedc = bed_contigs(A.bed);
    std::vector<std::string> filters;
    { std::istringstream ss(A.filter); std::string f; while (std::getline(ss, f, ',')) if (!f.empty()) filters.push_back(f); }
    std::vector<const char *> fptr;
    for (const auto &f : filters) fptr.push_back(f.c_str());
    const vio_params P = {A.min_qual, A.max_qual, A.max_size, A.cluster_gap};
    if (vio_read_vcf(A.query.c_str(), in.bed, &P, fptr.data(), int32_t(fptr.size()), &in.q)) die("ERROR: %s", vio_last_error());
    if (vio_read_vcf(A.truth.c_str(), in.bed, &P, fptr.data(), int32_t(fptr.size()), &in.t)) die("ERROR: %s", vio_last_error());
    in.q_read = in.q->vars; in.t_read = in.t->vars;
    if (vio_read_fasta(A.fasta.c_str(), &in.fa)) die("ERROR: %s", vio_last_error());
    for (int k = 0; k < in.q->n_ctg; k++) in.qn.push_back(in.q->ctg_name[k]);
    for (int k = 0; k < in.t->n_ctg; k++) in.tn.push_back(in.t->ctg_name[k]);
    for (int k = 0; k < in.fa->n_ctg; k++) in.fn.push_back(in.fa->ctg_name[k]);
}

// ---- which strata, in which order: the list's, the repeat and long repeat families', the context and the variant defaults
// A family of genome-wide k-mer strata (--stratify-repeats: include/vcfdist_repeats.h, --stratify-long-repeats:
// include/vcfdist_longrepeats.h): its option and its word in the messages, its entries and writer, and what its pass gave.  The
// near-repeat family (--stratify-near-repeats: include/vcfdist_nearrepeats.h) has no defaults and a spec type of its own: its
// entries are the parsed argument's (near_spec, with the names made of them), and its statistics carry the cost.
struct KmerFamily {
    bool Args::*on;
    const char *option, *word, *defaults_name;
    int (*defaults)(const vpr_repeat_stratum **, const char *const **, int32_t *);
    int (*intervals)(vpr_handle *, int32_t, const int64_t *, const uint8_t *, const vpr_repeat_stratum *, int32_t);
    int (*counts)(vpr_handle *, int64_t *);
    int (*download)(vpr_handle *, int32_t *, int32_t *);
    int (*stats)(vpr_handle *, int64_t *, int64_t *);
    int (*timing)(const vpr_handle *, double *, double *, double *, double *);
    decltype(&vrp_write_repeat_bed) write_bed;
    const vpr_repeat_stratum *spec = nullptr;
    const char *const *names = nullptr;
    int32_t n = 0;                                       // strata (0 without the option)
    std::vector<int64_t> off = {};                       // [n * FASTA contigs + 1], row = stratum * contigs + contig
    std::vector<int32_t> start = {}, stop = {};
    std::vector<int64_t> valid = {}, repeated = {};      // [n] starts
    double ms = 0;                                       // device ms of the pass
    std::vector<vpr_near_stratum> near_spec = {};        // the near-repeat family alone: its entries, its names, its compares and longest runs
    std::vector<std::string> near_names = {};
    std::vector<const char *> near_name_ptrs = {};
    std::vector<int64_t> compares = {}, max_run = {};
};
int long_repeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated) {
    int64_t n_last[VPR_LREP_MAX_SPEC];
    return vpr_longrepeat_stats(h, n_valid, n_repeated, n_last, nullptr);
}
struct StrataPlan : Pinned {
    std::vector<std::string> names;                      // every stratum in table order
    std::vector<vio_bed *> beds;                         // the list's BEDs
    int n_list = 0, n_bed = 0, n_pre = 0, n_strata = 0;  // strata up to the list's, the k-mer families', the context; all of them
    KmerFamily kmer[3] = {
        {&Args::stratify_repeats, "--stratify-repeats", "repeat", "vpr_repeats_default", vpr_repeats_default, vpr_repeat_intervals, vpr_repeat_interval_counts,
         vpr_repeat_download_intervals, vpr_repeat_stats, vpr_repeat_timing, vrp_write_repeat_bed},
        {&Args::stratify_long_repeats, "--stratify-long-repeats", "long repeat", "vpr_longrepeats_default", vpr_longrepeats_default, vpr_longrepeat_intervals,
         vpr_longrepeat_interval_counts, vpr_longrepeat_download_intervals, long_repeat_stats, vpr_longrepeat_timing, vrp_write_long_repeat_bed},
        {nullptr, "--stratify-near-repeats", "near repeat", nullptr, nullptr, nullptr, vpr_nearrepeat_interval_counts, vpr_nearrepeat_download_intervals,
         nullptr, vpr_nearrepeat_timing, vrp_write_near_repeat_bed}};
    const vpr_context_stratum *ctx_spec = nullptr; const vpr_variant_stratum *vs_spec = nullptr;
    const char *const *ctx_names = nullptr, *const *vs_names = nullptr;
    int32_t n_ctx = 0, n_vs = 0;
    // --stratify-derive, --stratify-cross (include/vcfdist_derive.h), behind every other stratum: their names, kinds and expressions
    // as derived-strata.tsv lists them, and the one call's programs
    struct Derived {
        std::vector<std::string> names, expressions;
        std::vector<int32_t> kinds, code_off = {0}, code;
        int n_cross = 0;
    } dv;
    int32_t n_dv = 0;
    ~StrataPlan() { for (vio_bed *b : beds) vio_bed_free(b); }
};
// --stratify: the strata list (GIAB format: name<TAB>path per line, blank and '#' lines skipped, a relative path is taken from
// the list's own directory) and its BEDs, each read and checked by vio_read_bed; any fault ends the run before anything is evaluated
void read_strata(const std::string &list, StrataPlan &S) {
    std::ifstream f(list);
    if (!f) die("ERROR: cannot open the strata list '%s'", list.c_str());
    const size_t sl = list.rfind('/');
    const std::string dir = sl == std::string::npos ? "" : list.substr(0, sl + 1);
    std::string line;
    int ln = 0;
    while (std::getline(f, line)) {
        ln++;
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        if (line.find_first_not_of(" \t") == std::string::npos || line[0] == '#') continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 >= line.size())
            die("ERROR: strata list '%s' line %d: expected name<TAB>path", list.c_str(), ln);
        const std::string name = line.substr(0, tab);
        std::string path = line.substr(tab + 1);
        if (path.find('\t') != std::string::npos) path = path.substr(0, path.find('\t'));
        if (std::find(S.names.begin(), S.names.end(), name) != S.names.end())
            die("ERROR: strata list '%s' line %d: duplicate stratum name '%s'", list.c_str(), ln, name.c_str());
        if (path[0] != '/') path = dir + path;
        vio_bed *b = nullptr;
        if (vio_read_bed(path.c_str(), &b)) die("ERROR: stratum '%s': %s", name.c_str(), vio_last_error());
        S.names.push_back(name); S.beds.push_back(b);
    }
    if (S.names.empty()) die("ERROR: strata list '%s' names no stratum", list.c_str());
}
// default strata behind the names there are; a name that is there already ends the run
void append_default_strata(std::vector<std::string> &names, const char *const *defaults, int n, const char *word, const char *option,
                           const std::string &list) {
    for (int k = 0; k < n; k++) {
        if (find(names, defaults[k]) >= 0)
            die("ERROR: strata list '%s': duplicate stratum name '%s' (a %s stratum of %s)", list.c_str(), defaults[k], word, option);
        names.push_back(defaults[k]);
    }
}
// --stratify-derive, --stratify-cross: every entry compiled by the library (one compiler for both command lines: its messages) against
// the names in front of it -- the derived entries in command-line order, then the crossed pairs, option by option
void derive_strata(const Args &A, StrataPlan &S) {
    if (S.names.empty()) {
        if (!A.derive.empty()) die("ERROR: --stratify-derive needs another --stratify* option");
        if (!A.cross.empty()) die("ERROR: --stratify-cross needs another --stratify* option");
        return;
    }
    StrataPlan::Derived &D = S.dv;
    auto add = [&](const char *option, const std::string &name, int32_t kind, const std::string &expression, const int32_t *code, int32_t n_code) {
        if (S.n_dv == VPR_DV_MAX_CLI) die("ERROR: %s: more than %d derived and crossed strata", option, VPR_DV_MAX_CLI);
        D.names.push_back(name); D.kinds.push_back(kind); D.expressions.push_back(expression);
        D.code.insert(D.code.end(), code, code + n_code);
        D.code_off.push_back(int32_t(D.code.size()));
        S.names.push_back(name); S.n_dv++;
    };
    std::vector<int32_t> code(VPR_DV_MAX_CODE), pairs(2 * VPR_DV_MAX_CLI);
    for (const std::string &entry : A.derive) {
        const std::vector<const char *> names = c_strs(S.names);
        std::vector<char> name(entry.size() + 1);
        int32_t n_code = 0;
        if (vpr_derive_compile(entry.c_str(), names.data(), int32_t(names.size()), name.data(), name.size(), code.data(), int32_t(code.size()), &n_code))
            die("ERROR: --stratify-derive: %s", vpr_derive_last_error());
        add("--stratify-derive", name.data(), VPR_DV_KIND_DERIVE, entry.substr(entry.find('=') + 1), code.data(), n_code);
    }
    for (const std::string &entry : A.cross) {
        const std::vector<const char *> names = c_strs(S.names);
        int32_t n_pairs = 0;
        if (vpr_derive_cross(entry.c_str(), names.data(), int32_t(names.size()), pairs.data(), VPR_DV_MAX_CLI, &n_pairs))
            die("ERROR: --stratify-cross: %s", vpr_derive_last_error());
        for (int32_t i = 0; i < n_pairs; i++) {
            const int32_t a = pairs[size_t(2 * i)], b = pairs[size_t(2 * i + 1)], and_ab[3] = {a, b, VPR_DV_AND};
            const std::string name = S.names[size_t(a)] + "&" + S.names[size_t(b)];
            add("--stratify-cross", name, VPR_DV_KIND_CROSS, name, and_ab, 3);
            D.n_cross++;
        }
    }
}
// the table order: the list's strata, the three k-mer families' (their intervals come from a genome-wide pass each in front of the
// contig loop and then travel with the list's rows), the default sequence-context strata, the default variant strata, the derived
// and the crossed strata
void plan_strata(const Args &A, StrataPlan &S) {
    if (!A.stratify.empty()) read_strata(A.stratify, S);
    S.n_list = int(S.names.size());
    for (KmerFamily &F : S.kmer) {
        if (!F.on) {             // the near-repeat family: the user's entries
            if (A.near.empty()) continue;
            F.near_spec = A.near;
            for (const vpr_near_stratum &sp : F.near_spec) {
                char buf[64];
                if (vpr_nearrepeat_name(&sp, buf, sizeof(buf))) die("ERROR: vpr_nearrepeat_name failed");
                F.near_names.push_back(buf);
            }
            F.near_name_ptrs = c_strs(F.near_names);
            F.names = F.near_name_ptrs.data(); F.n = int32_t(F.near_spec.size());
        } else {
            if (!(A.*F.on)) continue;
            if (F.defaults(&F.spec, &F.names, &F.n)) die("ERROR: %s failed", F.defaults_name);
        }
        append_default_strata(S.names, F.names, F.n, F.word, F.option, A.stratify);
    }
    S.n_bed = int(S.names.size());
    if (A.stratify_context) {
        if (vpr_context_default(&S.ctx_spec, &S.ctx_names, &S.n_ctx)) die("ERROR: vpr_context_default failed");
        append_default_strata(S.names, S.ctx_names, S.n_ctx, "sequence-context", "--stratify-context", A.stratify);
    }
    S.n_pre = int(S.names.size());
    if (A.stratify_variants) {
        if (vpr_varstrata_default(&S.vs_spec, &S.vs_names, &S.n_vs)) die("ERROR: vpr_varstrata_default failed");
        append_default_strata(S.names, S.vs_names, S.n_vs, "variant", "--stratify-variants", A.stratify);
    }
    derive_strata(A, S);
    S.n_strata = int(S.names.size());
}
// the genome-wide pass over all contigs of the FASTA, on a handle of its own: the evaluation has the memory back
void kmer_pass(KmerFamily &F, const vpr_config &cfg, const vio_fasta *fa) {
    if (!F.n) return;
    vpr_handle *hr = nullptr;
    if (vpr_create(&cfg, &hr)) { fprintf(stderr, "vpr_create: %s\n", vpr_last_error(nullptr)); exit(2); }
    F.off.assign(size_t(F.n) * size_t(fa->n_ctg) + 1, 0);
    const bool near = !F.near_spec.empty();
    if ((near ? vpr_nearrepeat_intervals(hr, fa->n_ctg, fa->ctg_off, fa->seq, F.near_spec.data(), F.n)
              : F.intervals(hr, fa->n_ctg, fa->ctg_off, fa->seq, F.spec, F.n)) || F.counts(hr, F.off.data()))
        die("ERROR: %s", vpr_last_error(hr));
    F.start.assign(size_t(F.off.back()) + 1, 0); F.stop.assign(size_t(F.off.back()) + 1, 0);
    F.valid.assign(size_t(F.n), 0); F.repeated.assign(size_t(F.n), 0);
    double ms[4] = {0, 0, 0, 0};
    F.compares.assign(size_t(F.n), 0); F.max_run.assign(size_t(F.n), 0);
    if (F.download(hr, F.start.data(), F.stop.data()) ||
        (near ? vpr_nearrepeat_stats(hr, F.valid.data(), F.repeated.data(), F.compares.data(), F.max_run.data()) : F.stats(hr, F.valid.data(), F.repeated.data())) ||
        F.timing(hr, &ms[0], &ms[1], &ms[2], &ms[3]))
        die("ERROR: %s", vpr_last_error(hr));
    F.ms = ms[0] + ms[1] + ms[2] + ms[3];
    vpr_destroy(hr);
}
// the rows of FASTA contig fi in all strata of the family, appended to a table of BED rows; off gets one entry per stratum
void kmer_rows(const KmerFamily &F, const vio_fasta *fa, int fi, std::vector<int32_t> &start, std::vector<int32_t> &stop, std::vector<int64_t> &off) {
    for (int k = 0; k < F.n; k++) {
        const size_t r = size_t(k) * size_t(fa->n_ctg) + size_t(fi);
        start.insert(start.end(), F.start.begin() + F.off[r], F.start.begin() + F.off[r + 1]);
        stop.insert(stop.end(), F.stop.begin() + F.off[r], F.stop.begin() + F.off[r + 1]);
        off.push_back(int64_t(start.size()));
    }
}
void kmer_report(const KmerFamily &F) {
    if (!F.n) return;
    std::string starts;
    for (int k = 0; k < F.n; k++) {
        char buf[128];
        if (F.near_spec.empty())
            snprintf(buf, sizeof(buf), "%lld valid and %lld repeated starts (k=%d), ", (long long)F.valid[size_t(k)], (long long)F.repeated[size_t(k)], F.spec[k].k);
        else
            snprintf(buf, sizeof(buf), "%lld valid and %lld near-repeated starts (k=%d, m=%d), ", (long long)F.valid[size_t(k)], (long long)F.repeated[size_t(k)],
                     F.near_spec[size_t(k)].k, F.near_spec[size_t(k)].m);
        starts += buf;
    }
    if (!F.near_spec.empty()) {
        long long compares = 0, longest = 0;
        for (int k = 0; k < F.n; k++) { compares += F.compares[size_t(k)]; longest = std::max<long long>(longest, F.max_run[size_t(k)]); }
        char buf[128];
        snprintf(buf, sizeof(buf), "%lld compares, longest run %lld, ", compares, longest);
        starts += buf;
    }
    fprintf(stderr, "[vcfdist_amd] %s strata: %lld intervals of %d strata, %s%.3f ms on the device\n", F.word, (long long)F.off.back(), F.n, starts.c_str(), F.ms);
}
// check_contigs (bed.cpp:135-284): the contigs to evaluate, in the order the reference's superclusterData walks them
std::vector<std::string> check_contigs(const std::vector<std::string> &q_in, const std::vector<std::string> &t_in,
                                       const std::vector<std::string> &fa, const std::vector<std::string> *bed) {
    std::vector<std::string> qc = q_in, tc = t_in;
    if (bed) {
        auto in_bed = [&](const std::string &c) { return find(*bed, c) >= 0; };
        qc.erase(std::remove_if(qc.begin(), qc.end(), [&](const std::string &c) { return !in_bed(c); }), qc.end());
        tc.erase(std::remove_if(tc.begin(), tc.end(), [&](const std::string &c) { return !in_bed(c); }), tc.end());
        for (const auto &c : qc) if (find(tc, c) < 0) warn("Contig '" + c + "' found in query VCF but not truth VCF.");
        for (const auto &c : tc) if (find(qc, c) < 0) warn("Contig '" + c + "' found in truth VCF but not query VCF.");
        for (const auto &c : *bed) {
            if (find(fa, c) < 0) die("ERROR: Contig '%s' found in BED but not reference FASTA.", c.c_str());
            if (find(qc, c) < 0) qc.push_back(c);
        }
        return qc;
    }
    for (const auto &c : tc) {
        if (find(fa, c) < 0) die("ERROR: Contig '%s' found in truth VCF but not reference FASTA. Please provide BED file.", c.c_str());
        if (find(qc, c) < 0) {
            warn("Contig '" + c + "' found in truth VCF but not query VCF. All truth variants on '" + c + "' will be false negatives.");
            qc.push_back(c);
        }
    }
    for (const auto &c : qc)
        if (find(tc, c) < 0) {
            warn("Contig '" + c + "' found in query VCF but not truth VCF. All query variants on '" + c + "' will be false positives.");
            if (find(fa, c) < 0) die("ERROR: contig '%s' not in reference FASTA", c.c_str());
        }
    return qc;
}
// superclusterData::transfer_phase_sets (cluster.cpp:186-330): one phase set per supercluster from the variants' PS -- the
// reference walks the superclusters, inside one the four haps (query 1, 2, truth 1, 2) and their variants, keeps one running
// maximum of PS per callset, and a variant whose PS exceeds its callset's maximum makes its PS the current phase set; a
// supercluster gets the phase set current at its end
std::vector<int32_t> transfer_phase_sets(const vio_hap_vars *const slot[4], const std::vector<int64_t> var_off[4], int n_sc) {
    int first_pos = -1, phase_set = 0;
    for (int i = 0; i < 4; i++)
        for (int v = 0; v < slot[i]->n; v++)
            if (slot[i]->phase_set[v]) {
                if (first_pos < 0 || slot[i]->pos[v] < first_pos) { first_pos = slot[i]->pos[v]; phase_set = slot[i]->phase_set[v]; }
                break;
            }
    std::vector<int32_t> out(size_t(n_sc), 0);
    int cur[2] = {0, 0};
    for (int k = 0; k < n_sc; k++) {
        for (int i = 0; i < 4; i++)
            for (int64_t v = var_off[i][size_t(k)]; v < var_off[i][size_t(k) + 1]; v++) {
                const int ps = slot[i]->phase_set[v];
                if (ps > cur[i >> 1]) { cur[i >> 1] = ps; phase_set = ps; }
            }
        out[size_t(k)] = phase_set;
    }
    return out;
}
// parameters.txt, write_params (print.cpp:30-56)
void write_params(const Args &A, const std::string &cmd) {
    FILE *f = fopen((A.prefix + "parameters.txt").c_str(), "w");
    if (!f) die("ERROR: cannot write %sparameters.txt", A.prefix.c_str());
    auto b2s = [](bool b) { return b ? "true" : "false"; };
    fprintf(f, "program = '%s'\nversion = '%s'\nout_prefix = '%s'\ncommand = '%s'\nreference_fasta = '%s'\n"
               "query_vcf = '%s'\ntruth_vcf = '%s'\nbed_file = '%s'\nwrite_outputs = %s\nfilters = '%s'\n"
               "min_var_qual = %d\nmax_var_qual = %d\nmax_var_size = %d\nsv_threshold = %d\n"
               "phase_threshold = %f\ncredit_threshold = %f\nrealign_truth = %s\nrealign_query = %s\n"
               "realign_only = %s\ncluster_method = '%s'\ncluster_min_gap = %d\n"
               "reach_min_gap = %d\nmax_cluster_itrs = %d\nmax_threads = %d\nmax_ram = %f\n"
               "sub = %d\nopen = %d\nextend = %d\neval_sub = %d\neval_open = %d\neval_extend = %d\ndistance = %s",
            "vcfdist_amd", vpr_version(), A.prefix.c_str(), cmd.c_str(), A.fasta.c_str(), A.query.c_str(), A.truth.c_str(), A.bed.c_str(), "true",
            A.filter.c_str(), A.min_qual, A.max_qual, A.max_size, A.sv_threshold, A.phase_threshold, A.credit_threshold, b2s(A.realign_truth),
            b2s(A.realign_query), b2s(A.realign_only), A.cluster.c_str(), A.cluster_gap, A.reach_min_gap, A.max_iterations, 64, 64.0, A.sub, A.open,
            A.extend, A.eval_sub, A.eval_open, A.eval_extend, b2s(A.distance));
    fclose(f);
}
// a callset's ##contig lines and both haps per contig, for vrp_write_vcf (variantData::write_vcf)
void write_callset_vcf(const std::string &path, const vio_callset *cs, const Inputs &in) {
    std::vector<vrp_vcf_contig> ctgs(size_t(cs->n_ctg));
    for (int k = 0; k < cs->n_ctg; k++) {
        vrp_vcf_contig &c = ctgs[size_t(k)];
        memset(&c, 0, sizeof(c));
        c.name = cs->ctg_name[k]; c.length = int32_t(cs->ctg_len[k]); c.ploidy = cs->ploidy[k];
        const int fi = find(in.fn, cs->ctg_name[k]);
        if (fi >= 0) { c.seq = in.seq(fi); c.seq_len = in.seq_len(fi); }
        for (int h = 0; h < 2; h++) hap_view(c.hap[h], cs->vars[2 * k + h]);
    }
    wrote(vrp_write_vcf(path.c_str(), ctgs.data(), cs->n_ctg, cs->sample, nullptr));
}
// the clusters of one hap as the run clusters: biWFA on the GPU (cluster.cpp:954-1263), or the distance rules (gap / size)
int cluster_hap(const vio_hap_vars &s, const uint8_t *seq, int64_t seq_len, const Args &A, vcl_clusters **cl) {
    if (A.cluster != "biwfa") {
        const vcl_hap hp = hap_cols(s);
        return vcl_simple_cluster(&hp, A.cluster == "size" ? 1 : 0, A.cluster_gap, A.reach_min_gap, cl);
    }
    const vcl_hap_seq hs = hap_seq(s);
    return vcl_wfa_cluster(&hs, seq, int32_t(seq_len), A.sub, A.open, A.extend, A.max_iterations, A.reach_min_gap, A.device, cl, nullptr);
}
// wf_swg_realign + left_shift of a whole callset (main.cpp:74-100): per contig and hap, cluster as the run clusters, then
// vrl_realign.  The callset's hap columns are pointed at the results, which in.realigned owns.
void realign_callset(const char *which, vio_callset *cs, Inputs &in, const Args &A, std::vector<vio_hap_vars> &cols) {
    cols.assign(size_t(2) * size_t(cs->n_ctg), EMPTY_HAP);
    int64_t n_cl = 0, n_in = 0, n_out = 0, n_edge = 0, n_limit = 0, n_error = 0;
    for (int k = 0; k < cs->n_ctg; k++) {
        const int fi = find(in.fn, cs->ctg_name[k]);
        if (fi < 0) die("ERROR: Contig '%s' not in reference FASTA (realignment of the %s VCF)", cs->ctg_name[k], which);
        for (int h = 0; h < 2; h++) {
            const vio_hap_vars *s = &cs->vars[2 * k + h];
            vcl_clusters *cl = nullptr;
            int rc = cluster_hap(*s, in.seq(fi), in.seq_len(fi), A, &cl);
            if (rc) die("ERROR: contig '%s': clustering the %s VCF failed (%d)", cs->ctg_name[k], which, rc);
            const vcl_hap_seq hs = hap_seq(*s);
            vrl_config rc_cfg = {A.sub, A.open, A.extend, A.max_qual, 0, 0};
            vrl_result *r = nullptr;
            rc = vrl_realign(&hs, s->var_qual, s->gt_qual, s->phase_set, s->orig_gt, cl, in.seq(fi), int32_t(in.seq_len(fi)), &rc_cfg, A.device, &r);
            vcl_clusters_free(cl);
            if (rc) die("ERROR: contig '%s': realigning the %s VCF failed (%d)", cs->ctg_name[k], which, rc);
            in.realigned.push_back(r);
            cols[size_t(2 * k + h)] = vio_hap_vars{r->n, r->pos, r->rlen, r->type, r->orig_gt, r->var_qual, r->gt_qual, r->phase_set,
                                                   r->ref_len, r->alt_len, r->ref_off, r->alt_off, r->pool, r->pool_len};
            n_cl += r->info.n_clusters; n_in += s->n; n_out += r->n;
            n_edge += r->info.n_edge; n_limit += r->info.n_limit; n_error += r->info.n_error;
        }
    }
    fprintf(stderr, "[vcfdist_amd] realigned %s VCF: %lld clusters, %lld -> %lld hap-variants\n", which, (long long)n_cl, (long long)n_in,
            (long long)n_out);
    if (n_edge + n_limit + n_error) {
        fprintf(stderr, "[WARN  vcfdist_amd] %s VCF: %lld cluster(s) NOT REALIGNED, their variants kept as read: %lld starting at the contig's "
                        "first base, %lld beyond the memory limit of one alignment, %lld with inconsistent variants\n",
                which, (long long)(n_edge + n_limit + n_error), (long long)n_edge, (long long)n_limit, (long long)n_error);
        if (A.strict) die("ERROR: %s VCF: %lld cluster(s) not realigned (--strict)", which, (long long)(n_edge + n_limit + n_error));
    }
    cs->vars = cols.data();
}
// realignment (main.cpp:50-180): the callsets as read, the contigs to evaluate, then each callset realigned in place of its
// columns.  With -ro the realigned callsets and the parameters (written first by the reference, main.cpp:35) are all there is.
std::vector<std::string> realign_inputs(const Args &A, Inputs &in, const std::string &cmd) {
    const bool write = !A.no_output_files;
    if (write && A.realign_query) write_callset_vcf(A.prefix + "orig-query.vcf", in.q, in);
    if (write && A.realign_truth) write_callset_vcf(A.prefix + "orig-truth.vcf", in.t, in);
    std::vector<std::string> contigs = check_contigs(in.qn, in.tn, in.fn, in.bed ? &in.bedc : nullptr);
    if (A.realign_query) {
        realign_callset("query", in.q, in, A, in.q_cols);
        if (A.realign_only && write) write_callset_vcf(A.prefix + "query.vcf", in.q, in);
    }
    if (A.realign_truth) realign_callset("truth", in.t, in, A, in.t_cols);
    if (A.realign_only) {
        if (A.realign_truth && write) write_callset_vcf(A.prefix + "truth.vcf", in.t, in);
        if (write) write_params(A, cmd);
    }
    return contigs;
}

// ---- what the run sums over the contigs
// A label pass (--classify-errors, --classify-matches): its entries and writers, its counts[2][4][VPR_EC_CLASSES / VPR_MK_KINDS][nq] summed over
// the contigs (empty without the option), with --cut-classes the same [n_strata][...] and [n_rep][...] (empty without it), the device ms
struct LabelPass {
    const char *noun;
    bool Args::*option;
    size_t labels;
    int (*label)(vpr_handle *, const vpr_variants *, const int32_t *, const Args &, int64_t *);
    int (*timing)(const vpr_handle *, double *);
    int (*write)(const char *, const int64_t *, const int64_t *, int32_t, int32_t);
    int (*cut_strata)(vpr_handle *, int32_t, int32_t, int64_t *);
    int (*cut_boot)(vpr_handle *, int32_t, int32_t, const uint64_t *, uint64_t, int32_t, int32_t, int64_t *);
    int (*cut_timing)(const vpr_handle *, double *, double *);
    int (*write_strata)(const char *, const char *const *, int32_t, const int64_t *, const int64_t *, int32_t, int32_t);
    int (*write_boot)(const char *, const int64_t *, const int64_t *, const int64_t *, int32_t, int32_t, int32_t);
    std::vector<int64_t> total = {}, strata = {}, boot = {};
    double ms = 0, cut_ms = 0;
};
int label_errors(vpr_handle *h, const vpr_variants *V, const int32_t *pb, const Args &A, int64_t *c) {
    return vpr_errclass(h, V, nullptr, pb, A.error_window, A.min_qual, A.max_qual, c);
}
int label_matches(vpr_handle *h, const vpr_variants *V, const int32_t *pb, const Args &A, int64_t *c) {
    return vpr_matchkind(h, V, nullptr, pb, A.min_qual, A.max_qual, c);
}
// One contig: prepare_contig fills the head, evaluate_contig the results, and it is kept until the writers have run
struct Contig : Pinned {
    std::string name;
    size_t ordinal = 0;              // among the evaluated contigs: the high word of its superclusters' bootstrap keys
    int fi = -1, ploidy = 0, n_sc = 0, n_clusters = 0;                   // (fi: its index in the FASTA)
    const uint8_t *seq = nullptr;
    int64_t ctg_off[2] = {0, 0}, length = 0, n_hapvars = 0;
    const vio_hap_vars *slot[4];
    vcl_superclusters *sc = nullptr;
    // what the evaluation works on and lets go when done: variant offsets per supercluster, bootstrap keys, the path's view of the contig
    std::vector<int64_t> var_off[4];
    std::vector<int32_t> sc_ctg;
    std::vector<uint64_t> keys;
    vpr_variants V;
    vpr_results res;
    void *res_block = nullptr;       // (res points into it)
    std::vector<int32_t> phase_sets, pb, sw, fl, phase_block;
    // -d: the contig's edit records (vpr_distance_download)
    std::vector<int32_t> e_sc, e_pos, e_len, e_minq, e_maxq;
    std::vector<uint8_t> e_hap, e_type;
    Contig() { memset(&res, 0, sizeof(res)); memset(&V, 0, sizeof(V)); }
    ~Contig() { if (res_block) vpr_host_free(res_block); if (sc) vcl_superclusters_free(sc); }
};
struct Totals {
    std::vector<int64_t> total, strat_total;             // counts[2][4][3][nq]; --stratify*: counts[n_strata][2][4][3][nq]
    int64_t strat_vars = 0, strat_none = 0;              // hap-variants seen / in no stratum
    std::vector<int64_t> vs_query, vs_truth;             // variant-strata.tsv: members per callset
    std::vector<int64_t> dv_query, dv_truth;             // derived-strata.tsv: the same
    std::vector<std::string> ctx_contigs;                // context-strata.bed: contigs, rows contig-major
    std::vector<int64_t> ctx_off = {0};
    std::vector<int32_t> ctx_start, ctx_stop;
    std::vector<int64_t> boot_total, boot_strat;         // --bootstrap: counts[n_rep][2][4][3][nq], with strata also [n_strata][n_rep][...]
    double vs_ms = 0, dv_ms = 0, ctx_ms = 0, boot_ms = 0;    // device ms of the launches
    LabelPass pass[2] = {
        {"error classes", &Args::classify_errors, VPR_EC_CLASSES, label_errors, vpr_errclass_timing, vrp_write_error_classes, vpr_errclass_strata,
         vpr_errclass_boot, vpr_errclass_cut_timing, vrp_write_error_classes_stratified, vrp_write_error_classes_bootstrap},
        {"match kinds", &Args::classify_matches, VPR_MK_KINDS, label_matches, vpr_matchkind_timing, vrp_write_match_kinds, vpr_matchkind_strata,
         vpr_matchkind_boot, vpr_matchkind_cut_timing, vrp_write_match_kinds_stratified, vrp_write_match_kinds_bootstrap}};
    vpr_pr_row rows[2 * VPR_VARTYPES];                   // the PRECISION-RECALL SUMMARY
    std::deque<Contig> outs;
    Totals(const Args &A, const StrataPlan &S) {
        total.assign(size_t(2) * VPR_VARTYPES * 3 * size_t(A.max_qual - A.min_qual + 1), 0);
        strat_total.assign(total.size() * size_t(S.n_strata), 0);
        vs_query.assign(size_t(S.n_vs), 0); vs_truth.assign(size_t(S.n_vs), 0);
        dv_query.assign(size_t(S.n_dv), 0); dv_truth.assign(size_t(S.n_dv), 0);
        boot_total.assign(total.size() * size_t(A.bootstrap), 0); boot_strat.assign(boot_total.size() * size_t(S.n_strata), 0);
        for (LabelPass &P : pass) {
            const bool on = A.*P.option;
            P.total.assign(on ? total.size() / 3 * P.labels : 0, 0);
            P.strata.assign(on && A.cut_classes ? P.total.size() * size_t(S.n_strata) : 0, 0);
            P.boot.assign(on && A.cut_classes ? P.total.size() * size_t(A.bootstrap) : 0, 0);
        }
    }
};
struct Run { const Args &A; const Inputs &in; const StrataPlan &S; Totals &T; vpr_handle *h; };      // what every stage reads, and the sums it adds to
void check(const Run &R, const Contig &c, int rc) { if (rc) die("ERROR: contig '%s': %s", c.name.c_str(), vpr_last_error(R.h)); }      // every call on the run's handle
// a contig's header length and ploidy (superclusterData ctor, cluster.cpp:134-157): the query's header wins, then the truth's
void contig_header(const Inputs &in, int qi, int ti, int64_t seq_len, Contig &C) {
    if (qi >= 0) { C.length = in.q->ctg_len[qi]; C.ploidy = in.q->ploidy[qi]; }
    else if (ti >= 0) { C.length = in.t->ctg_len[ti]; C.ploidy = in.t->ploidy[ti]; }
    else { C.length = seq_len; C.ploidy = 0; }
}
// the four hap slots, clustering, superclustering (cluster.cpp:404-808), the variant offsets per supercluster, and the path's view of it all
void prepare_contig(const Run &R, const std::string &ctg, size_t ordinal, Contig &c) {
    const Args &A = R.A; const Inputs &in = R.in;
    c.name = ctg; c.ordinal = ordinal;
    c.fi = find(in.fn, ctg);
    if (c.fi < 0) die("ERROR: contig '%s' not in reference FASTA", ctg.c_str());
    c.seq = in.seq(c.fi); c.ctg_off[1] = in.seq_len(c.fi);
    const int qi = find(in.qn, ctg), ti = find(in.tn, ctg);
    c.slot[0] = qi >= 0 ? &in.q->vars[2 * qi] : &EMPTY_HAP; c.slot[1] = qi >= 0 ? &in.q->vars[2 * qi + 1] : &EMPTY_HAP;
    c.slot[2] = ti >= 0 ? &in.t->vars[2 * ti] : &EMPTY_HAP; c.slot[3] = ti >= 0 ? &in.t->vars[2 * ti + 1] : &EMPTY_HAP;
    contig_header(in, qi, ti, c.ctg_off[1], c);
    vcl_hap haps[4]; vcl_clusters *cl[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; i++) {
        haps[i] = hap_cols(*c.slot[i]);
        const int rc = cluster_hap(*c.slot[i], c.seq, c.ctg_off[1], A, &cl[i]);
        if (rc) die("ERROR: contig '%s': clustering failed (%d)", ctg.c_str(), rc);
        c.n_clusters += cl[i]->n; c.n_hapvars += c.slot[i]->n;
    }
    if (vcl_supercluster(haps, cl, A.max_supercluster_size, &c.sc)) die("ERROR: contig '%s': superclustering failed", ctg.c_str());
    for (int i = 0; i < 4; i++) vcl_clusters_free(cl[i]);     // (c.sc holds its own tables)
    const vcl_superclusters *sc = c.sc; c.n_sc = sc->n;
    for (int i = 0; i < 4; i++) {
        c.var_off[i].assign(size_t(c.n_sc) + 1, 0);
        const vcl_clusters *k = sc->clusters[i];
        if (k->n > 0) for (int j = 0; j <= c.n_sc; j++) c.var_off[i][size_t(j)] = k->var_beg[sc->brk[i][j]];
    }
    vpr_variants &V = c.V;
    V.n_ctg = 1; V.ctg_off = c.ctg_off; V.ctg_seq = c.seq;
    for (int i = 0; i < 4; i++) V.var_off[i] = c.var_off[i].data();
    if (!c.n_sc) return;             // (no variant: the contig alone is what context_only sends)
    c.sc_ctg.assign(size_t(c.n_sc), 0);
    V.n_sc = c.n_sc; V.sc_ctg = c.sc_ctg.data(); V.sc_beg = sc->beg; V.sc_end = sc->end;
    for (int i = 0; i < 4; i++) {
        const vio_hap_vars *s = c.slot[i];
        V.var_pos[i] = s->pos; V.var_type[i] = s->type; V.var_qual[i] = s->var_qual;
        V.var_ref_off[i] = s->ref_off; V.var_ref_len[i] = s->ref_len; V.var_alt_off[i] = s->alt_off; V.var_alt_len[i] = s->alt_len;
        V.allele_pool[i] = pool_of(*s);
    }
    c.keys.assign(size_t(c.n_sc), 0);
    for (int k = 0; k < c.n_sc; k++) c.keys[size_t(k)] = (uint64_t(c.ordinal) << 32) | uint64_t(k);
}
// -d: edits_wrapper for this contig's superclusters, behind the precision/recall path (main.cpp:223-238)
void distance_contig(const Run &R, Contig &c) {
    const Args &A = R.A;
    vpr_dist_config dc; memset(&dc, 0, sizeof(dc));
    dc.eval_sub = A.eval_sub; dc.eval_open = A.eval_open; dc.eval_extend = A.eval_extend; dc.min_qual = A.min_qual; dc.max_qual = A.max_qual;
    vpr_dist_info di;
    check(R, c, vpr_distance(R.h, &c.V, &dc) || vpr_distance_info(R.h, &di));
    const size_t ne = size_t(di.n_edits);
    c.e_sc.resize(ne); c.e_pos.resize(ne); c.e_len.resize(ne); c.e_minq.resize(ne); c.e_maxq.resize(ne); c.e_hap.resize(ne); c.e_type.resize(ne);
    std::vector<int64_t> qd(size_t(A.max_qual) + 2);
    vpr_dist_results dr; memset(&dr, 0, sizeof(dr));
    dr.qual_dists = qd.data(); dr.edit_sc = c.e_sc.data(); dr.edit_hap = c.e_hap.data(); dr.edit_pos = c.e_pos.data();
    dr.edit_type = c.e_type.data(); dr.edit_len = c.e_len.data(); dr.edit_min_qual = c.e_minq.data(); dr.edit_max_qual = c.e_maxq.data();
    check(R, c, vpr_distance_download(R.h, &dr));
    if (di.n_limit || di.n_error)
        fprintf(stderr, "[WARN  vcfdist_amd] contig '%s': %lld distance alignment(s) beyond the device's memory plan and %lld that failed: "
                        "NOT EVALUATED -- left out of the distance metrics\n", c.name.c_str(), (long long)di.n_limit, (long long)di.n_error);
    fprintf(stderr, "[vcfdist_amd] %s: %lld distance alignments, %lld edits, edit distance %lld\n", c.name.c_str(), (long long)di.n_jobs,
            (long long)di.n_edits, (long long)*std::min_element(qd.begin(), qd.end()));
}
// the same evaluation, its FP and FN cut by why they are wrong, its TP by how they were matched (the classes are resident)
void label_contig(const Run &R, Contig &c) {
    for (LabelPass &P : R.T.pass) {
        if (P.total.empty()) continue;
        std::vector<int64_t> n(P.total.size(), 0); double ms = 0;
        check(R, c, P.label(R.h, &c.V, c.pb.data(), R.A, n.data()) || P.timing(R.h, &ms));
        add_into(P.total.data(), n.data(), n.size());
        P.ms += ms;
    }
}
// the context intervals of the contig the last vpr_context_masks saw, appended to the table of context-strata.bed
void keep_context_intervals(const Run &R, const Contig &c) {
    Totals &T = R.T; const int n_ctx = R.S.n_ctx;
    std::vector<int64_t> off(size_t(n_ctx) + 1, 0);
    check(R, c, vpr_context_interval_counts(R.h, off.data()));
    const size_t at = T.ctx_start.size(), n = size_t(off[size_t(n_ctx)]);
    T.ctx_start.resize(at + n + 1); T.ctx_stop.resize(at + n + 1);
    check(R, c, vpr_context_download_intervals(R.h, T.ctx_start.data() + at, T.ctx_stop.data() + at));
    T.ctx_start.resize(at + n); T.ctx_stop.resize(at + n);
    for (int k = 1; k <= n_ctx; k++) T.ctx_off.push_back(int64_t(at) + off[size_t(k)]);
    T.ctx_contigs.push_back(c.name);
    double ms = 0, ms_mask = 0;
    (void)vpr_context_timing(R.h, &ms, &ms_mask); T.ctx_ms += ms;
}
// the same evaluation, cut by region: membership words, then the histogram per stratum
void stratify_contig(const Run &R, Contig &c) {
    const Args &A = R.A; const StrataPlan &S = R.S; Totals &T = R.T;
    std::vector<int64_t> iv_off(1, 0);                   // the list's rows of this contig, then the k-mer families': ordinary BED rows
    std::vector<int32_t> iv_start, iv_stop;
    for (int k = 0; k < S.n_list; k++) {
        int64_t n = 0; const int32_t *st = nullptr, *sp = nullptr;
        if (vio_bed_intervals(S.beds[size_t(k)], c.name.c_str(), &n, &st, &sp)) die("ERROR: %s", vio_last_error());
        iv_start.insert(iv_start.end(), st, st + n); iv_stop.insert(iv_stop.end(), sp, sp + n);
        iv_off.push_back(int64_t(iv_start.size()));
    }
    for (const KmerFamily &F : S.kmer) kmer_rows(F, R.in.fa, c.fi, iv_start, iv_stop, iv_off);
    const vpr_strata ST = {S.n_bed, 1, iv_off.data(), iv_start.data(), iv_stop.data()};
    // (with --stratify-context the context intervals are built on the device and go to the same mask kernel)
    if (S.n_pre) check(R, c, S.n_ctx ? vpr_context_masks(R.h, &c.V, S.n_bed ? &ST : nullptr, S.ctx_spec, S.n_ctx) : vpr_strata_masks(R.h, &c.V, &ST));
    // (with --stratify-variants the bits made from the variant tables follow in the same words)
    if (S.n_vs) {
        double ms = 0;
        check(R, c, vpr_varstrata_masks(R.h, &c.V, S.vs_spec, S.n_vs, S.n_pre ? 1 : 0) || vpr_varstrata_timing(R.h, &ms));
        T.vs_ms += ms;
    }
    // (with --stratify-derive / --stratify-cross one call on the bits that are there appends theirs)
    if (S.n_dv) {
        double ms = 0;
        check(R, c, vpr_derive_masks(R.h, S.dv.code_off.data(), S.dv.code.data(), S.n_dv) || vpr_derive_timing(R.h, &ms));
        T.dv_ms += ms;
    }
    std::vector<int64_t> counts(T.strat_total.size(), 0);
    check(R, c, vpr_pr_counts_strata(R.h, nullptr, c.pb.data(), A.min_qual, A.max_qual, counts.data()));
    add_into(T.strat_total.data(), counts.data(), counts.size());
    const size_t n_words = (size_t(S.n_strata) + 63) / 64;
    std::vector<uint64_t> words[4]; uint64_t *wp[4];
    for (int i = 0; i < 4; i++) { words[i].assign(std::max<size_t>(n_words * size_t(c.slot[i]->n), 1), 0); wp[i] = words[i].data(); }
    check(R, c, vpr_strata_download_masks(R.h, wp));
    if (S.n_ctx) keep_context_intervals(R, c);
    for (int i = 0; i < 4; i++) {
        const size_t nv = size_t(c.slot[i]->n);
        for (size_t v = 0; v < nv; v++) {
            uint64_t any = 0;
            for (size_t w = 0; w < n_words; w++) any |= words[i][w * nv + v];
            T.strat_none += any == 0;
            for (int k = 0; k < S.n_vs; k++)
                (i < 2 ? T.vs_query : T.vs_truth)[size_t(k)] += int64_t(words[i][size_t((S.n_pre + k) >> 6) * nv + v] >> ((S.n_pre + k) & 63) & 1);
            for (int k = 0, at = S.n_pre + S.n_vs; k < S.n_dv; k++, at++)
                (i < 2 ? T.dv_query : T.dv_truth)[size_t(k)] += int64_t(words[i][size_t(at >> 6) * nv + v] >> (at & 63) & 1);
        }
        T.strat_vars += int64_t(nv);
    }
}
// the same evaluation, resampled over superclusters (after the masks: a pass per stratum cuts by them)
void bootstrap_contig(const Run &R, Contig &c) {
    const Args &A = R.A; Totals &T = R.T;
    std::vector<int64_t> rep(T.boot_total.size(), 0);
    for (int k = -1; k < R.S.n_strata; k++) {
        int32_t grid[3]; double ms = 0;
        check(R, c, vpr_pr_counts_boot(R.h, nullptr, c.pb.data(), A.min_qual, A.max_qual, c.keys.data(), A.bootstrap_seed, A.bootstrap, k, rep.data()) ||
                        vpr_boot_info(R.h, grid, &ms));
        add_into(k < 0 ? T.boot_total.data() : T.boot_strat.data() + size_t(k) * rep.size(), rep.data(), rep.size());
        T.boot_ms += ms;
    }
}
// the labels of the same evaluation cut and resampled: their bytes and the words are both resident now
void cut_contig(const Run &R, Contig &c) {
    const Args &A = R.A;
    for (LabelPass &P : R.T.pass) {
        if (P.total.empty()) continue;
        double ms_strata = 0, ms_boot = 0; std::vector<int64_t> n(std::max(P.strata.size(), P.boot.size()), 0);
        if (R.S.n_strata) {
            check(R, c, P.cut_strata(R.h, A.min_qual, A.max_qual, n.data()) || P.cut_timing(R.h, &ms_strata, &ms_boot));
            add_into(P.strata.data(), n.data(), P.strata.size());
            P.cut_ms += ms_strata;
        }
        if (A.bootstrap) {
            check(R, c, P.cut_boot(R.h, A.min_qual, A.max_qual, c.keys.data(), A.bootstrap_seed, A.bootstrap, -1, n.data()) ||
                            P.cut_timing(R.h, &ms_strata, &ms_boot));
            add_into(P.boot.data(), n.data(), P.boot.size());
            P.cut_ms += ms_boot;
        }
    }
}

const uint32_t ERR_BITS = VPR_ST_ERR_LIMIT | VPR_ST_ERR_NO_PTR | VPR_ST_ERR_UNFINISHED;      // an alignment the GPU path did not evaluate

// the reference's WARN lines (dist.cpp:1203-1223) and -- loudly -- what this implementation did not evaluate
void print_warnings(const Run &R, const Contig &c) {
    const uint32_t *status = c.res.aln_status;
    static const struct { uint32_t bit; const char *text; } W[] = {
        {VPR_ST_WARN_REF_ED, "Nonzero reference edit distance with no truth variants at ctg %s supercluster %d"},
        {VPR_ST_WARN_QUERY_ED, "Query edit distance changed with no query variants at ctg %s supercluster %d"},
        {VPR_ST_WARN_EXCEEDS, "Query edit distance exceeds reference edit distance at ctg %s supercluster %d"},
        {VPR_ST_WARN_ZERO_ED, "Zero edit distance with truth variants at ctg %s supercluster %d"}};
    for (const auto &w : W)
        for (int a = 0; a < 4 * c.n_sc; a++)
            if (status[a] & w.bit) { fputs("[WARN  vcfdist] ", stderr); fprintf(stderr, w.text, c.name.c_str(), a / 4); fputc('\n', stderr); }
    int n_bad = 0;
    for (int k = 0; k < c.n_sc; k++) n_bad += ((status[4 * k] | status[4 * k + 1] | status[4 * k + 2] | status[4 * k + 3]) & ERR_BITS) != 0;
    if (n_bad) {
        fprintf(stderr, "[WARN  vcfdist_amd] contig '%s': %d supercluster(s) with alignments beyond an implementation limit of the GPU path: "
                        "NOT EVALUATED -- their variants are left out of every count and table\n", c.name.c_str(), n_bad);
        if (R.A.strict) die("ERROR: contig '%s': %d supercluster(s) not evaluated (--strict)", c.name.c_str(), n_bad);
    }
}
// no superclusters: the writers still want the per-variant columns (there are no variants); context-strata.bed, its intervals alone
void context_only(const Run &R, Contig &c) {
    vpr_results &res = c.res;
    static uint8_t zero8[1]; static int32_t zero32[1]; static float zerof[1];
    for (int i = 0; i < 4; i++)
        for (int w = 0; w < 2; w++) {
            res.errtype[i][w] = zero8; res.sync_group[i][w] = zero32; res.credit[i][w] = zerof;
            res.ref_ed[i][w] = zero32; res.query_ed[i][w] = zero32; res.callq[i][w] = zerof;
        }
    res.sc_phase = zero32; res.orig_phase_dist = zero32; res.swap_phase_dist = zero32;
    if (!R.S.n_ctx) return;
    check(R, c, vpr_context_masks(R.h, &c.V, nullptr, R.S.ctx_spec, R.S.n_ctx));
    keep_context_intervals(R, c);
}
// One contig on the handle.  The entries read what earlier calls left resident there, so the order is the contract:
//   1. vpr_upload_variants -> vpr_execute -> vpr_results_alloc / vpr_download;  2. -d: vpr_distance* (distance_contig)
//   3. status masking -> vpr_phase -> vpr_pr_counts (this makes the variant classes resident)
//   4. vpr_errclass / vpr_matchkind (label_contig: the label bytes become resident)
//   5. the masks: vpr_context_masks or vpr_strata_masks, then vpr_varstrata_masks and vpr_derive_masks appended behind them (stratify_contig)
//   6. vpr_pr_counts_strata -> vpr_strata_download_masks -> the context intervals (stratify_contig, keep_context_intervals)
//   7. vpr_pr_counts_boot for the whole contig and every stratum (bootstrap_contig);  8. the label cuts (cut_contig)
//   9. the warnings (print_warnings)
// A contig without a supercluster makes none of these calls but the context masks (context_only).
void evaluate_contig(const Run &R, Contig &c) {
    const Args &A = R.A; Totals &T = R.T; const int n_sc = c.n_sc;
    if (n_sc > 0) {
        check(R, c, vpr_upload_variants(R.h, &c.V) || vpr_execute(R.h));
        check(R, c, vpr_results_alloc(R.h, &c.res, &c.res_block) || vpr_download(R.h, &c.res));
        if (A.distance) distance_contig(R, c);
        // a supercluster with an alignment the GPU path did not evaluate takes no side in the contig's phasing
        for (int a = 0; a < 4 * n_sc; a++) if (c.res.aln_status[a] & ERR_BITS) c.res.sc_phase[a >> 2] = VPR_PHASE_NONE;
        c.phase_sets = transfer_phase_sets(c.slot, c.var_off, n_sc);
        c.pb.assign(size_t(n_sc), 0); c.sw.assign(size_t(n_sc), 0); c.fl.assign(size_t(n_sc), 0);
        int32_t ns = 0, nf = 0;
        if (vpr_phase(c.res.sc_phase, c.phase_sets.data(), n_sc, c.pb.data(), c.sw.data(), &ns, c.fl.data(), &nf))
            die("ERROR: contig '%s': unexpected phase", c.name.c_str());
        c.sw.resize(size_t(ns)); c.fl.resize(size_t(nf));
        std::vector<uint8_t> cls[4]; const uint8_t *clsp[4];
        for (int i = 0; i < 4; i++) {
            const vio_hap_vars *s = c.slot[i];
            cls[i].assign(size_t(std::max(s->n, 1)), 0);
            if (s->n) vpr_var_class(s->type, s->ref_len, s->alt_len, s->n, A.sv_threshold, cls[i].data());
            clsp[i] = cls[i].data();
        }
        std::vector<int64_t> counts(T.total.size(), 0);
        check(R, c, vpr_pr_counts(R.h, clsp, c.pb.data(), A.min_qual, A.max_qual, counts.data()));
        add_into(T.total.data(), counts.data(), counts.size());
        label_contig(R, c);
        if (R.S.n_strata) stratify_contig(R, c);
        if (A.bootstrap) bootstrap_contig(R, c);
        if (A.cut_classes) cut_contig(R, c);
        print_warnings(R, c);
    } else context_only(R, c);
    fprintf(stderr, "[vcfdist_amd] %s: %lld hap-variants, %d clusters, %d superclusters, %zu switch / %zu flip errors\n", c.name.c_str(),
            (long long)c.n_hapvars, c.n_clusters, n_sc, c.sw.size(), c.fl.size());
    c.phase_block.assign(size_t(n_sc) + 1, 0);
    const int32_t n_pb = vrp_phase_blocks(c.phase_sets.data(), n_sc, c.phase_block.data());
    c.phase_block.resize(size_t(std::max(n_pb, 0)) + 1);
    for (auto &v : c.var_off) v = {};      // (the writers do not want the working set)
    c.sc_ctg = {}; c.keys = {}; memset(&c.V, 0, sizeof(c.V));
}

// ---- after the contigs: the files and the closing lines
// -d: write_distance (printed even with -n), write_edits (edit.cpp:134-280)
void write_distance(const Run &R) {
    const Args &A = R.A;
    std::vector<vrp_edits> sets;
    for (const Contig &C : R.T.outs)
        sets.push_back(vrp_edits{C.name.c_str(), int64_t(C.e_sc.size()), C.e_sc.data(), C.e_hap.data(), C.e_pos.data(), C.e_type.data(),
                                 C.e_len.data(), C.e_minq.data(), C.e_maxq.data()});
    std::vector<char> text(size_t(1) << 16);
    const int n = vrp_write_distance(A.prefix.c_str(), sets.data(), int32_t(sets.size()), A.min_qual, A.max_qual, A.eval_sub, A.eval_open,
                                     A.eval_extend, 1, A.no_output_files ? 0 : 1, text.data(), int64_t(text.size()));
    wrote(n < 0);
    if (!A.no_output_files) wrote(vrp_write_edits((A.prefix + "edits.tsv").c_str(), sets.data(), int32_t(sets.size())));
    printf("%s\n", text.data());
}
// the contigs as the per-variant writers take them
std::vector<vrp_contig> contig_table(const Run &R) {
    std::vector<vrp_contig> ctgs(R.T.outs.size());
    for (size_t k = 0; k < ctgs.size(); k++) {
        const Contig &C = R.T.outs[k];
        vrp_contig &c = ctgs[k];
        memset(&c, 0, sizeof(c));
        const int fi = find(R.in.fn, C.name);
        c.name = C.name.c_str(); c.length = int32_t(C.length); c.ploidy = C.ploidy;
        c.seq = R.in.seq(fi); c.seq_len = R.in.seq_len(fi);
        for (int i = 0; i < 4; i++) {
            vrp_hap &hp = c.hap[i];
            hap_view(hp, *C.slot[i]); hp.phase_set = C.slot[i]->phase_set;
            hp.n_cluster = C.sc->clusters[i]->n;
            hp.cluster_beg = C.sc->clusters[i]->n ? C.sc->clusters[i]->var_beg : nullptr;
            for (int w = 0; w < 2; w++) {
                hp.errtype[w] = C.res.errtype[i][w]; hp.credit[w] = C.res.credit[i][w]; hp.sync_group[w] = C.res.sync_group[i][w];
                hp.ref_ed[w] = C.res.ref_ed[i][w]; hp.query_ed[w] = C.res.query_ed[i][w];
            }
            c.sc_brk[i] = C.sc->brk[i];
        }
        c.n_sc = C.sc->n; c.sc_beg = C.sc->beg; c.sc_end = C.sc->end;
        c.sc_phase = C.res.sc_phase; c.pb_phase = C.pb.data(); c.orig_phase_dist = C.res.orig_phase_dist; c.swap_phase_dist = C.res.swap_phase_dist;
        c.sc_phase_set = C.phase_sets.data(); c.n_pb = int32_t(C.phase_block.size()) - 1; c.phase_block = C.phase_block.data();
        c.n_switches = int32_t(C.sw.size()); c.n_flips = int32_t(C.fl.size()); c.switches = C.sw.data(); c.flips = C.fl.data();
    }
    return ctgs;
}

void write_outputs(const Run &R, const std::string &cmd, const std::vector<std::string> &contigs) {
    const Args &A = R.A; const StrataPlan &S = R.S; const Totals &T = R.T;
    const char *pre = A.prefix.c_str();
    const std::vector<const char *> names = c_strs(S.names);
    wrote(vrp_write_precision_recall(pre, T.total.data(), A.min_qual, A.max_qual));
    write_params(A, cmd);
    if (S.n_strata) {      // the stratified tables, and what lists the strata that were built here (the evaluated contigs in evaluation order, rows contig-major)
        const std::vector<const char *> cn = c_strs(contigs), ctx_cn = c_strs(T.ctx_contigs);
        wrote(vrp_write_stratified(pre, names.data(), S.n_strata, T.strat_total.data(), A.min_qual, A.max_qual));
        if (A.bootstrap)
            wrote(vrp_write_bootstrap_stratified(pre, names.data(), S.n_strata, T.strat_total.data(), T.boot_strat.data(), A.bootstrap, A.bootstrap_seed,
                                                 A.min_qual, A.max_qual));
        for (const KmerFamily &F : S.kmer) {           // repeat-strata.bed, long-repeat-strata.bed, near-repeat-strata.bed
            if (!F.n) continue;
            std::vector<int64_t> off(1, 0);
            std::vector<int32_t> st, sp;
            for (const auto &c : contigs) kmer_rows(F, R.in.fa, find(R.in.fn, c), st, sp, off);
            st.push_back(0); sp.push_back(0);      // (never empty: a pointer is wanted)
            wrote(F.write_bed(pre, cn.data(), int32_t(cn.size()), F.names, F.n, off.data(), st.data(), sp.data()));
        }
        if (S.n_ctx)
            wrote(vrp_write_context_bed(pre, ctx_cn.data(), int32_t(ctx_cn.size()), S.ctx_names, S.n_ctx, T.ctx_off.data(), T.ctx_start.data(), T.ctx_stop.data()));
        if (S.n_vs) wrote(vrp_write_variant_strata(pre, S.vs_names, S.vs_spec, S.n_vs, T.vs_query.data(), T.vs_truth.data()));
        if (S.n_dv)
            wrote(vrp_write_derived_strata(pre, c_strs(S.dv.names).data(), S.dv.kinds.data(), c_strs(S.dv.expressions).data(), S.n_dv, T.dv_query.data(),
                                           T.dv_truth.data()));
    }
    for (const LabelPass &P : T.pass)
        if (!P.total.empty()) wrote(P.write(pre, P.total.data(), T.total.data(), A.min_qual, A.max_qual));
    if (A.bootstrap) wrote(vrp_write_bootstrap(pre, T.total.data(), T.boot_total.data(), A.bootstrap, A.bootstrap_seed, A.min_qual, A.max_qual));
    for (const LabelPass &P : T.pass) {
        if (!A.cut_classes || P.total.empty()) continue;
        if (S.n_strata) wrote(P.write_strata(pre, names.data(), S.n_strata, P.strata.data(), T.strat_total.data(), A.min_qual, A.max_qual));
        if (A.bootstrap) wrote(P.write_boot(pre, P.total.data(), T.total.data(), P.boot.data(), A.bootstrap, A.min_qual, A.max_qual));
    }
    const std::vector<vrp_contig> ctgs = contig_table(R); const int32_t n = int32_t(ctgs.size());
    auto path = [&](const char *name) { return A.prefix + name; };
    wrote(vrp_write_phase_blocks(path("phase-blocks.tsv").c_str(), ctgs.data(), n) || vrp_write_switchflips(path("switchflips.tsv").c_str(), ctgs.data(), n) ||
          vrp_write_phasing_summary(path("phasing-summary.tsv").c_str(), ctgs.data(), n) || vrp_write_superclusters(path("superclusters.tsv").c_str(), ctgs.data(), n) ||
          vrp_write_variants(path("query.tsv").c_str(), ctgs.data(), n, 0) || vrp_write_variants(path("truth.tsv").c_str(), ctgs.data(), n, 1) ||
          vrp_write_summary_vcf(path("summary.vcf").c_str(), ctgs.data(), n, cmd.c_str(), nullptr, float(A.credit_threshold)));
    if (A.realign_query) write_callset_vcf(A.prefix + "query.vcf", R.in.q, R.in);
    if (A.realign_truth) write_callset_vcf(A.prefix + "truth.vcf", R.in.t, R.in);
}
// the closing lines of every option on stderr, and the PRECISION-RECALL SUMMARY
void report(const Run &R) {
    const Args &A = R.A; const StrataPlan &S = R.S; const Totals &T = R.T;
    const LabelPass &ec = T.pass[0], &mk = T.pass[1]; const size_t nq = size_t(A.max_qual - A.min_qual + 1);
    if (S.n_strata)
        fprintf(stderr, "[vcfdist_amd] stratified: %d strata, %lld of %lld hap-variants in none of them\n", S.n_strata, (long long)T.strat_none,
                (long long)T.strat_vars);
    for (const KmerFamily &F : S.kmer) kmer_report(F);
    if (S.n_ctx)
        fprintf(stderr, "[vcfdist_amd] context strata: %lld intervals of %d strata, %.3f ms on the device\n", (long long)T.ctx_start.size(), S.n_ctx, T.ctx_ms);
    if (S.n_vs) fprintf(stderr, "[vcfdist_amd] variant strata: %d strata, %.3f ms on the device\n", S.n_vs, T.vs_ms);
    if (S.n_dv)
        fprintf(stderr, "[vcfdist_amd] derived strata: %d strata (%d derived, %d crossed), %.3f ms on the device\n", S.n_dv, S.n_dv - S.dv.n_cross, S.dv.n_cross,
                T.dv_ms);
    if (A.classify_errors) {      // the classified errors at threshold NONE: the ALL rows' classes of both callsets
        long long n_fp = 0, n_fn = 0;
        for (int c = 0; c < VPR_EC_CLASSES; c++) {
            n_fp += ec.total[((size_t(0) * VPR_VARTYPES + VPR_VARTYPE_ALL) * VPR_EC_CLASSES + size_t(c)) * nq];
            n_fn += ec.total[((size_t(1) * VPR_VARTYPES + VPR_VARTYPE_ALL) * VPR_EC_CLASSES + size_t(c)) * nq];
        }
        fprintf(stderr, "[vcfdist_amd] error classes: window %d, %lld query FP and %lld truth FN classified, %.3f ms on the device\n", A.error_window,
                n_fp, n_fn, ec.ms);
    }
    if (A.classify_matches) {     // the matched variants at threshold NONE: the ALL rows' kinds of both callsets
        long long n[2][VPR_MK_KINDS];
        for (int cs = 0; cs < 2; cs++)
            for (int c = 0; c < VPR_MK_KINDS; c++) n[cs][c] = mk.total[((size_t(cs) * VPR_VARTYPES + VPR_VARTYPE_ALL) * VPR_MK_KINDS + size_t(c)) * nq];
        fprintf(stderr, "[vcfdist_amd] match kinds: query TP %lld exact, %lld shifted, %lld regrouped, %lld partial; truth TP %lld exact, %lld shifted, "
                "%lld regrouped, %lld partial, %.3f ms on the device\n", n[0][0], n[0][1], n[0][2], n[0][3], n[1][0], n[1][1], n[1][2], n[1][3], mk.ms);
    }
    if (A.cut_classes)
        for (const LabelPass &P : T.pass) {
            if (P.total.empty()) continue;
            std::string what;
            if (S.n_strata) what += std::to_string(S.n_strata) + " strata, ";
            if (A.bootstrap) what += std::to_string(A.bootstrap) + " replicates, ";
            fprintf(stderr, "[vcfdist_amd] %s cut: %s%.3f ms on the device\n", P.noun, what.c_str(), P.cut_ms);
        }
    if (A.bootstrap)
        fprintf(stderr, "[vcfdist_amd] bootstrap: %d replicates, seed %llu, %.3f ms on the device\n", A.bootstrap, (unsigned long long)A.bootstrap_seed, T.boot_ms);
    printf("PRECISION-RECALL SUMMARY\n\n");
    printf("TYPE\tTHRESHOLD\tTRUTH_TP\tQUERY_TP\tTRUTH_FN\tQUERY_FP\tPREC\t\tRECALL\t\tF1_SCORE\tF1_QSCORE\n");
    static const char *NAMES[] = {"SNP", "INDEL", "SV", "ALL"};
    for (const vpr_pr_row &r : T.rows) {
        printf("%s\t%s Q >= %-2d\t%-16d%-16d%-16d%-16d%f\t%f\t%f\t%f\n", NAMES[r.vartype], r.best ? "BEST" : "NONE", r.qual, r.truth_tp, r.query_tp,
               r.truth_fn, r.query_fp, r.precision, r.recall, r.f1_score, r.f1_qscore);
        if (r.best) printf("\n");
    }
}

}  // namespace

int main(int argc, char **argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);        // (before HIP starts: include/vcfdist_pr.h, vpr_select_device)
    const Args A = parse(argc, argv);
    std::string cmd = "vcfdist";
    for (int i = 1; i < argc; i++) { cmd += " "; cmd += argv[i]; }
    (void)vpr_select_device(A.device);

    Inputs in; StrataPlan S;
    if (!A.bed.empty() && vio_read_bed(A.bed.c_str(), &in.bed)) die("ERROR: %s", vio_last_error());
    plan_strata(A, S);          // (behind the -b BED, in front of the callsets: a fault of the strata ends the run before they are read)
    read_inputs(A, in);
    const std::vector<std::string> contigs = realign_inputs(A, in, cmd);
    if (A.realign_only) return 0;

    Totals T(A, S);
    vpr_config cfg; memset(&cfg, 0, sizeof(cfg));
    cfg.device = A.device; cfg.max_qual = float(A.max_qual); cfg.credit_threshold = A.credit_threshold; cfg.phase_threshold = A.phase_threshold;
    cfg.band_mode = 1;
    for (KmerFamily &F : S.kmer) kmer_pass(F, cfg, in.fa);
    vpr_handle *h = nullptr;
    if (vpr_create(&cfg, &h)) { fprintf(stderr, "vpr_create: %s\n", vpr_last_error(nullptr)); return 2; }

    const Run R = {A, in, S, T, h};
    for (size_t k = 0; k < contigs.size(); k++) {
        T.outs.emplace_back();
        prepare_contig(R, contigs[k], k, T.outs.back());
        evaluate_contig(R, T.outs.back());
    }

    if (A.distance) write_distance(R);
    if (vpr_pr_summary(T.total.data(), A.min_qual, A.max_qual, T.rows)) die("ERROR: vpr_pr_summary failed");
    if (!A.no_output_files) write_outputs(R, cmd, contigs);
    report(R);
    T.outs.clear();             // (the results' pinned blocks go before the handle does)
    vpr_destroy(h);
    return 0;
}
