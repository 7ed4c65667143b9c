// main.cpp -- vcfdist_gpu: the reference's command line for the precision/recall evaluation with the host orchestration in C++
// (main.cpp / globals.cpp of vcfdist v2.6.4: parse the arguments, read the VCFs / BED / FASTA, per contig cluster -> supercluster
// -> precision_recall_wrapper -> phase, then the counters, the PRECISION-RECALL SUMMARY and the output files) over the C ABIs of
// this repository: include/vcfdist_io.h (readers), vcfdist_cluster.h (clustering on the GPU / host, superclustering),
// vcfdist_pr.h (the alignment path on the GPU: generate_ptrs_strs on the device, vpr_execute, phasing, counters),
// vcfdist_report.h (writers).  One process, one GPU; the sharded runs (one process per GPU, RCCL) are `python -m vcfdist_amd`
// under torch.distributed.run, which is the same sequence of calls.  No CPU fallback: without a HIP device vpr_create fails.
//
//   vcfdist_gpu <query.vcf[.gz]> <truth.vcf[.gz]> <ref.fasta[.gz]> [-b regions.bed] [-p prefix] [-n] [-c biwfa | gap N | size N]
//               [-l max variant size] [-s max supercluster size] [-mn / -mx qual] [-f filters] [-i iterations] [-x -o -e penalties]
//               [-ct credit threshold] [-pt phasing threshold] [-sv threshold] [--reach-min-gap N] [--strict] [--device N]
//               [-d] [-ex -eo -ee evaluation penalties] [-rq] [-rt] [-ro] [--stratify strata.tsv] [--stratify-repeats] [--stratify-long-repeats] [--stratify-context]
//               [--stratify-variants]
//               [--bootstrap N] [--bootstrap-seed S]
//               [--classify-errors] [--error-window N]
//               [--classify-matches]
//               [--cut-classes]
// With -d the distance metrics (edits_wrapper, dist.cpp:1908-2077) run on the GPU after each contig's precision/recall path
// (include/vcfdist_distance.h), as the reference's main.cpp:223-238 runs them after precision_recall_threads_wrapper.
// With -rq / -rt a callset is clustered and realigned on the GPU (include/vcfdist_realign.h) before the evaluation, in the order of
// the reference's main.cpp:50-180 (orig-*.vcf, realign query, realign truth; -ro stops there and writes query.vcf / truth.vcf).
// With --stratify FILE (the GIAB list format: one name<TAB>path of a BED per line) the counters of the one evaluation are also cut
// by region on the GPU (include/vcfdist_strata.h): stratified-precision-recall.tsv and stratified-precision-recall-summary.tsv.
// With --stratify-context the default sequence-context strata (homopolymers, short tandem repeats, GC bands: intervals built on
// the GPU from the FASTA, include/vcfdist_context.h) follow the list's strata, or stand alone; context-strata.bed holds them.
// With --stratify-repeats the default repeat strata (where the FASTA is not unique: include/vcfdist_repeats.h, one genome-wide pass
// on the GPU before the contig loop) follow the list's strata, in front of the context strata; repeat-strata.bed holds them.
// With --stratify-long-repeats the default long repeat strata (repeated 64-, 100- and 250-mers: include/vcfdist_longrepeats.h, one
// more genome-wide pass) follow those, in front of the context strata; long-repeat-strata.bed holds them.
// With --stratify-variants the default variant strata (transitions / transversions, indel size bins, hom / het, isolated / crowded:
// bits made on the GPU from the variant tables, include/vcfdist_varstrata.h) follow those, or stand alone; variant-strata.tsv lists
// them with their numbers of members.
// With --classify-errors every query FP and truth FN gets the first error class that applies (include/vcfdist_errclass.h: right
// allele with the wrong genotype, on the aligned or on the other haplotype, another allele at the site, something within
// --error-window N bases (default 50), nothing), joined across the callsets on the GPU: error-classes.tsv, error-classes-summary.tsv.
// With --classify-matches every TP of either callset gets the first match kind that applies (include/vcfdist_matchkind.h: exact --
// what an allele-for-allele comparison finds --, shifted, regrouped, partial), from the resident sync groups on the GPU:
// match-kinds.tsv, match-kinds-summary.tsv.
// With --cut-classes (beside --classify-errors / --classify-matches and a --stratify* option or --bootstrap) the label counts of
// every active pass are cut by the strata and resampled as well, from the label bytes and the membership words that are resident
// after the passes (include/vcfdist_labelcut.h): stratified-error-classes.tsv, stratified-error-classes-summary.tsv,
// bootstrap-error-classes-summary.tsv and their match-kinds counterparts.  Without the option no file changes.
// With --bootstrap N the counters are resampled N times on the GPU (include/vcfdist_bootstrap.h: a Poisson bootstrap over
// superclusters, conditional on the phasing): bootstrap-precision-recall-summary.tsv with 95 % percentile intervals,
// bootstrap-replicates.tsv, and with --stratify stratified-bootstrap-precision-recall-summary.tsv.
#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
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
#include "../../include/vcfdist_strata.h"
#include "../../include/vcfdist_varstrata.h"
#include "../../include/vcfdist_errclass.h"
#include "../../include/vcfdist_matchkind.h"

namespace {

struct Args {
    std::string query, truth, fasta, bed, filter, prefix = "./", cluster = "biwfa", stratify;
    bool stratify_context = false, stratify_variants = false, stratify_repeats = false, stratify_long_repeats = false;
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
        else if (o == "--stratify-variants") a.stratify_variants = true;
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
    if (a.cut_classes && a.stratify.empty() && !a.stratify_repeats && !a.stratify_long_repeats && !a.stratify_context && !a.stratify_variants && !a.bootstrap)
        die("ERROR: --cut-classes needs --stratify, --stratify-context, --stratify-variants or --bootstrap");
    if ((a.realign_query || a.realign_truth) && (a.sub < 1 || a.extend < 1))
        die("ERROR: realignment needs a mismatch penalty (-x) and a gap-extension penalty (-e) of at least 1");
    return a;
}

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

// --stratify: the strata list (GIAB format: name<TAB>path per line, blank and '#' lines skipped, a relative path is taken from
// the list's own directory) and its BEDs, each read and checked by vio_read_bed; any fault ends the run before anything is evaluated
struct Strata { std::vector<std::string> names; std::vector<vio_bed *> beds; };
Strata read_strata(const std::string &list) {
    Strata S;
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
    return S;
}

int find(const std::vector<std::string> &v, const std::string &s) {
    for (size_t i = 0; i < v.size(); i++) if (v[i] == s) return int(i);
    return -1;
}

// A family of genome-wide k-mer strata (--stratify-repeats: include/vcfdist_repeats.h, --stratify-long-repeats:
// include/vcfdist_longrepeats.h): its option and its word in the messages, its entries and writer, and what its pass gave.
struct KmerFamily {
    bool on;
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
    std::vector<int64_t> off;                            // [n * FASTA contigs + 1], row = stratum * contigs + contig
    std::vector<int32_t> start, stop;
    std::vector<int64_t> valid, repeated;                // [n] starts
    double ms = 0;                                       // device ms of the pass
};
int long_repeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated) {
    int64_t n_last[VPR_LREP_MAX_SPEC];
    return vpr_longrepeat_stats(h, n_valid, n_repeated, n_last, nullptr);
}
// the family's default strata behind the names there are; a name that is there already ends the run
void kmer_register(KmerFamily &F, const std::string &list, std::vector<std::string> &names) {
    if (!F.on) return;
    if (F.defaults(&F.spec, &F.names, &F.n)) die("ERROR: %s failed", F.defaults_name);
    for (int k = 0; k < F.n; k++) {
        if (find(names, F.names[k]) >= 0)
            die("ERROR: strata list '%s': duplicate stratum name '%s' (a %s stratum of %s)", list.c_str(), F.names[k], F.word, F.option);
        names.push_back(F.names[k]);
    }
}
// the genome-wide pass over all contigs of the FASTA, on a handle of its own: the evaluation has the memory back
void kmer_pass(KmerFamily &F, const vpr_config &cfg, const vio_fasta *fa) {
    if (!F.n) return;
    vpr_handle *hr = nullptr;
    if (vpr_create(&cfg, &hr)) { fprintf(stderr, "vpr_create: %s\n", vpr_last_error(nullptr)); exit(2); }
    F.off.assign(size_t(F.n) * size_t(fa->n_ctg) + 1, 0);
    if (F.intervals(hr, fa->n_ctg, fa->ctg_off, fa->seq, F.spec, F.n) || F.counts(hr, F.off.data())) die("ERROR: %s", vpr_last_error(hr));
    F.start.assign(size_t(F.off.back()) + 1, 0); F.stop.assign(size_t(F.off.back()) + 1, 0);
    F.valid.assign(size_t(F.n), 0); F.repeated.assign(size_t(F.n), 0);
    double ms[4] = {0, 0, 0, 0};
    if (F.download(hr, F.start.data(), F.stop.data()) || F.stats(hr, F.valid.data(), F.repeated.data()) || F.timing(hr, &ms[0], &ms[1], &ms[2], &ms[3]))
        die("ERROR: %s", vpr_last_error(hr));
    F.ms = ms[0] + ms[1] + ms[2] + ms[3];
    vpr_destroy(hr);
}
void kmer_report(const KmerFamily &F) {
    if (!F.n) return;
    std::string starts;
    for (int k = 0; k < F.n; k++) {
        char buf[128];
        snprintf(buf, sizeof(buf), "%lld valid and %lld repeated starts (k=%d), ", (long long)F.valid[size_t(k)], (long long)F.repeated[size_t(k)], F.spec[k].k);
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
std::vector<int32_t> transfer_phase_sets(const vio_hap_vars *slot[4], const std::vector<int64_t> var_off[4], int n_sc) {
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

struct ContigOut {       // what the writers need of one contig, kept alive until they have run
    std::string name;
    int64_t length = 0;
    int ploidy = 0;
    const vio_hap_vars *slot[4];
    vcl_superclusters *sc = nullptr;
    vpr_results res;
    void *res_block = nullptr;
    std::vector<int32_t> phase_sets, pb, sw, fl, phase_block;
    // -d: the contig's edit records (vpr_distance_download)
    std::vector<int32_t> e_sc, e_pos, e_len, e_minq, e_maxq;
    std::vector<uint8_t> e_hap, e_type;
};

const vio_hap_vars EMPTY_HAP = {0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};

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
void write_callset_vcf(const std::string &path, const vio_callset *cs, const vio_fasta *fa, const std::vector<std::string> &fn) {
    std::vector<vrp_vcf_contig> ctgs(size_t(cs->n_ctg));
    static const uint8_t no_pool[1] = {0};
    for (int k = 0; k < cs->n_ctg; k++) {
        vrp_vcf_contig &c = ctgs[size_t(k)];
        memset(&c, 0, sizeof(c));
        c.name = cs->ctg_name[k]; c.length = int32_t(cs->ctg_len[k]); c.ploidy = cs->ploidy[k];
        const int fi = find(fn, cs->ctg_name[k]);
        if (fi >= 0) { c.seq = fa->seq + fa->ctg_off[fi]; c.seq_len = fa->ctg_off[fi + 1] - fa->ctg_off[fi]; }
        for (int h = 0; h < 2; h++) {
            const vio_hap_vars &v = cs->vars[2 * k + h];
            vrp_hap &hp = c.hap[h];
            hp.n_var = v.n; hp.pos = v.pos; hp.type = v.type; hp.var_qual = v.var_qual; hp.ref_len = v.ref_len; hp.alt_len = v.alt_len;
            hp.ref_off = v.ref_off; hp.alt_off = v.alt_off; hp.pool = v.pool ? v.pool : no_pool;
        }
    }
    if (vrp_write_vcf(path.c_str(), ctgs.data(), cs->n_ctg, cs->sample, nullptr)) die("ERROR: %s", vrp_last_error());
}

// wf_swg_realign + left_shift of a whole callset (main.cpp:74-100): per contig and hap, cluster as the run clusters (biWFA on the
// GPU, or gap / size), then vrl_realign.  The callset's hap columns are pointed at the results, which `keep` owns.
void realign_callset(const char *which, vio_callset *cs, const vio_fasta *fa, const std::vector<std::string> &fn, const Args &A,
                     std::vector<vrl_result *> &keep, std::vector<vio_hap_vars> &cols) {
    cols.assign(size_t(2) * size_t(cs->n_ctg), EMPTY_HAP);
    int64_t n_cl = 0, n_in = 0, n_out = 0, n_edge = 0, n_limit = 0, n_error = 0;
    for (int k = 0; k < cs->n_ctg; k++) {
        const int fi = find(fn, cs->ctg_name[k]);
        if (fi < 0) die("ERROR: Contig '%s' not in reference FASTA (realignment of the %s VCF)", cs->ctg_name[k], which);
        const uint8_t *seq = fa->seq + fa->ctg_off[fi];
        const int64_t seq_len = fa->ctg_off[fi + 1] - fa->ctg_off[fi];
        for (int h = 0; h < 2; h++) {
            const vio_hap_vars *s = &cs->vars[2 * k + h];
            const vcl_hap hp = {s->n, s->pos, s->rlen, s->type, s->ref_len, s->alt_len};
            static const uint8_t no_pool[1] = {0};
            const vcl_hap_seq hs = {hp, s->ref_off, s->alt_off, s->pool ? s->pool : no_pool};
            vcl_clusters *cl = nullptr;
            int rc = A.cluster == "biwfa"
                         ? vcl_wfa_cluster(&hs, seq, int32_t(seq_len), A.sub, A.open, A.extend, A.max_iterations, A.reach_min_gap, A.device, &cl, nullptr)
                         : vcl_simple_cluster(&hp, A.cluster == "size" ? 1 : 0, A.cluster_gap, A.reach_min_gap, &cl);
            if (rc) die("ERROR: contig '%s': clustering the %s VCF failed (%d)", cs->ctg_name[k], which, rc);
            vrl_config rc_cfg = {A.sub, A.open, A.extend, A.max_qual, 0, 0};
            vrl_result *r = nullptr;
            rc = vrl_realign(&hs, s->var_qual, s->gt_qual, s->phase_set, s->orig_gt, cl, seq, int32_t(seq_len), &rc_cfg, A.device, &r);
            vcl_clusters_free(cl);
            if (rc) die("ERROR: contig '%s': realigning the %s VCF failed (%d)", cs->ctg_name[k], which, rc);
            keep.push_back(r);
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

}  // namespace

int main(int argc, char **argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);        // (before HIP starts: include/vcfdist_pr.h, vpr_select_device)
    const Args A = parse(argc, argv);
    std::string cmd = "vcfdist";
    for (int i = 1; i < argc; i++) { cmd += " "; cmd += argv[i]; }
    (void)vpr_select_device(A.device);

    vio_bed *bed = nullptr;
    std::vector<std::string> bedc;
    if (!A.bed.empty()) {
        if (vio_read_bed(A.bed.c_str(), &bed)) die("ERROR: %s", vio_last_error());
        bedc = bed_contigs(A.bed);
    }
    Strata strata;
    if (!A.stratify.empty()) strata = read_strata(A.stratify);
    // --stratify-repeats: the default repeat strata (include/vcfdist_repeats.h) behind the list's; their intervals come from one
    // genome-wide pass in front of the contig loop and then travel with the list's rows
    // --stratify-long-repeats: the default long repeat strata (include/vcfdist_longrepeats.h) behind those, from a genome-wide pass
    // of their own; their rows travel the same way
    const int n_list = int(strata.names.size());
    KmerFamily kmer[2] = {};
    kmer[0].on = A.stratify_repeats; kmer[0].option = "--stratify-repeats"; kmer[0].word = "repeat";
    kmer[0].defaults_name = "vpr_repeats_default"; kmer[0].defaults = vpr_repeats_default; kmer[0].intervals = vpr_repeat_intervals;
    kmer[0].counts = vpr_repeat_interval_counts; kmer[0].download = vpr_repeat_download_intervals; kmer[0].stats = vpr_repeat_stats;
    kmer[0].timing = vpr_repeat_timing; kmer[0].write_bed = vrp_write_repeat_bed;
    kmer[1].on = A.stratify_long_repeats; kmer[1].option = "--stratify-long-repeats"; kmer[1].word = "long repeat";
    kmer[1].defaults_name = "vpr_longrepeats_default"; kmer[1].defaults = vpr_longrepeats_default; kmer[1].intervals = vpr_longrepeat_intervals;
    kmer[1].counts = vpr_longrepeat_interval_counts; kmer[1].download = vpr_longrepeat_download_intervals; kmer[1].stats = long_repeat_stats;
    kmer[1].timing = vpr_longrepeat_timing; kmer[1].write_bed = vrp_write_long_repeat_bed;
    for (KmerFamily &F : kmer) kmer_register(F, A.stratify, strata.names);
    // --stratify-context: the default sequence-context strata (include/vcfdist_context.h) behind the list's and the repeat strata
    const int n_bed = int(strata.names.size());
    const vpr_context_stratum *ctx_spec = nullptr;
    const char *const *ctx_names = nullptr;
    int32_t n_ctx = 0;
    if (A.stratify_context) {
        if (vpr_context_default(&ctx_spec, &ctx_names, &n_ctx)) die("ERROR: vpr_context_default failed");
        for (int k = 0; k < n_ctx; k++) {
            if (find(strata.names, ctx_names[k]) >= 0)
                die("ERROR: strata list '%s': duplicate stratum name '%s' (a sequence-context stratum of --stratify-context)", A.stratify.c_str(), ctx_names[k]);
            strata.names.push_back(ctx_names[k]);
        }
    }
    // --stratify-variants: the default variant strata (include/vcfdist_varstrata.h) behind the list's and the context strata
    const int n_pre = int(strata.names.size());
    const vpr_variant_stratum *vs_spec = nullptr;
    const char *const *vs_names = nullptr;
    int32_t n_vs = 0;
    if (A.stratify_variants) {
        if (vpr_varstrata_default(&vs_spec, &vs_names, &n_vs)) die("ERROR: vpr_varstrata_default failed");
        for (int k = 0; k < n_vs; k++) {
            if (find(strata.names, vs_names[k]) >= 0)
                die("ERROR: strata list '%s': duplicate stratum name '%s' (a variant stratum of --stratify-variants)", A.stratify.c_str(), vs_names[k]);
            strata.names.push_back(vs_names[k]);
        }
    }
    std::vector<int64_t> vs_query(size_t(n_vs), 0), vs_truth(size_t(n_vs), 0);    // variant-strata.tsv: members per callset
    double vs_ms = 0;
    const int n_strata = int(strata.names.size());
    std::vector<std::string> ctx_contigs;                                       // context-strata.bed: contigs, rows contig-major
    std::vector<int64_t> ctx_off(1, 0);
    std::vector<int32_t> ctx_start, ctx_stop;
    double ctx_ms = 0;
    // the context intervals of the contig the last vpr_context_masks saw, appended to the table of context-strata.bed
    auto keep_context_intervals = [&](vpr_handle *h, const std::string &ctg) {
        std::vector<int64_t> off(size_t(n_ctx) + 1, 0);
        if (vpr_context_interval_counts(h, off.data())) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
        const size_t at = ctx_start.size(), n = size_t(off[size_t(n_ctx)]);
        ctx_start.resize(at + n + 1); ctx_stop.resize(at + n + 1);
        if (vpr_context_download_intervals(h, ctx_start.data() + at, ctx_stop.data() + at)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
        ctx_start.resize(at + n); ctx_stop.resize(at + n);
        for (int k = 1; k <= n_ctx; k++) ctx_off.push_back(int64_t(at) + off[size_t(k)]);
        ctx_contigs.push_back(ctg);
        double ms = 0, ms_mask = 0;
        (void)vpr_context_timing(h, &ms, &ms_mask);
        ctx_ms += ms;
    };
    std::vector<std::string> filters;
    { std::istringstream ss(A.filter); std::string f; while (std::getline(ss, f, ',')) if (!f.empty()) filters.push_back(f); }
    std::vector<const char *> fptr;
    for (const auto &f : filters) fptr.push_back(f.c_str());
    const vio_params P = {A.min_qual, A.max_qual, A.max_size, A.cluster_gap};
    vio_callset *q = nullptr, *t = nullptr;
    vio_fasta *fa = nullptr;
    if (vio_read_vcf(A.query.c_str(), bed, &P, fptr.data(), int32_t(fptr.size()), &q)) die("ERROR: %s", vio_last_error());
    if (vio_read_vcf(A.truth.c_str(), bed, &P, fptr.data(), int32_t(fptr.size()), &t)) die("ERROR: %s", vio_last_error());
    if (vio_read_fasta(A.fasta.c_str(), &fa)) die("ERROR: %s", vio_last_error());
    std::vector<std::string> qn, tn, fn;
    for (int k = 0; k < q->n_ctg; k++) qn.push_back(q->ctg_name[k]);
    for (int k = 0; k < t->n_ctg; k++) tn.push_back(t->ctg_name[k]);
    for (int k = 0; k < fa->n_ctg; k++) fn.push_back(fa->ctg_name[k]);
    const bool write = !A.no_output_files;
    // realignment (main.cpp:50-180): the callsets as read, then each realigned in place of its columns
    if (write && A.realign_query) write_callset_vcf(A.prefix + "orig-query.vcf", q, fa, fn);
    if (write && A.realign_truth) write_callset_vcf(A.prefix + "orig-truth.vcf", t, fa, fn);
    const std::vector<std::string> contigs = check_contigs(qn, tn, fn, bed ? &bedc : nullptr);
    vio_hap_vars *q_read = q->vars, *t_read = t->vars;
    std::vector<vrl_result *> realigned;
    std::vector<vio_hap_vars> q_cols, t_cols;
    if (A.realign_query) {
        realign_callset("query", q, fa, fn, A, realigned, q_cols);
        if (A.realign_only && write) write_callset_vcf(A.prefix + "query.vcf", q, fa, fn);
    }
    if (A.realign_truth) realign_callset("truth", t, fa, fn, A, realigned, t_cols);
    auto release_realigned = [&]() {
        q->vars = q_read; t->vars = t_read;
        for (vrl_result *r : realigned) vrl_result_free(r);
        realigned.clear();
    };
    if (A.realign_only) {          // realign only: the parameters (written first by the reference, main.cpp:35) and stop
        if (A.realign_truth && write) write_callset_vcf(A.prefix + "truth.vcf", t, fa, fn);
        if (write) write_params(A, cmd);
        release_realigned();
        vio_callset_free(q); vio_callset_free(t); vio_fasta_free(fa);
        if (bed) vio_bed_free(bed);
        for (vio_bed *b : strata.beds) vio_bed_free(b);
        return 0;
    }

    const int nq = A.max_qual - A.min_qual + 1;
    std::vector<int64_t> total(size_t(2) * VPR_VARTYPES * 3 * size_t(nq), 0);
    std::vector<int64_t> strat_total(total.size() * size_t(n_strata), 0);      // --stratify: counts[n_strata][2][4][3][nq]
    int64_t strat_vars = 0, strat_none = 0;                                     // hap-variants seen / in no stratum
    // --classify-errors, --classify-matches: counts[2][4][VPR_EC_CLASSES / VPR_MK_KINDS][nq] summed over the contigs (empty
    // without the option); device ms of the launches
    struct LabelPass {
        std::vector<int64_t> total;
        double ms;
        int (*timing)(const vpr_handle *, double *);
        int (*write)(const char *, const int64_t *, const int64_t *, int32_t, int32_t);
        // --cut-classes: the same counts [n_strata][...] and [n_rep][...] (empty without it), the entries, the writers, device ms
        const char *noun;
        std::vector<int64_t> strata, boot;
        double cut_ms;
        int (*cut_strata)(vpr_handle *, int32_t, int32_t, int64_t *);
        int (*cut_boot)(vpr_handle *, int32_t, int32_t, const uint64_t *, uint64_t, int32_t, int32_t, int64_t *);
        int (*cut_timing)(const vpr_handle *, double *, double *);
        int (*write_strata)(const char *, const char *const *, int32_t, const int64_t *, const int64_t *, int32_t, int32_t);
        int (*write_boot)(const char *, const int64_t *, const int64_t *, const int64_t *, int32_t, int32_t, int32_t);
    };
    auto label_pass = [&](bool on, size_t labels) {
        LabelPass P{};
        P.total.assign(on ? total.size() / 3 * labels : 0, 0);
        P.strata.assign(on && A.cut_classes ? P.total.size() * size_t(n_strata) : 0, 0);
        P.boot.assign(on && A.cut_classes ? P.total.size() * size_t(A.bootstrap) : 0, 0);
        return P;
    };
    LabelPass ec = label_pass(A.classify_errors, VPR_EC_CLASSES), mk = label_pass(A.classify_matches, VPR_MK_KINDS);
    ec.timing = vpr_errclass_timing; ec.write = vrp_write_error_classes; ec.noun = "error classes";
    ec.cut_strata = vpr_errclass_strata; ec.cut_boot = vpr_errclass_boot; ec.cut_timing = vpr_errclass_cut_timing;
    ec.write_strata = vrp_write_error_classes_stratified; ec.write_boot = vrp_write_error_classes_bootstrap;
    mk.timing = vpr_matchkind_timing; mk.write = vrp_write_match_kinds; mk.noun = "match kinds";
    mk.cut_strata = vpr_matchkind_strata; mk.cut_boot = vpr_matchkind_boot; mk.cut_timing = vpr_matchkind_cut_timing;
    mk.write_strata = vrp_write_match_kinds_stratified; mk.write_boot = vrp_write_match_kinds_bootstrap;
    // --bootstrap: counts[n_rep][2][4][3][nq], with --stratify also [n_strata][n_rep][2][4][3][nq]; device ms of the launches
    std::vector<int64_t> boot_total(total.size() * size_t(A.bootstrap), 0), boot_strat(boot_total.size() * size_t(n_strata), 0);
    double boot_ms = 0;
    vpr_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.device = A.device; cfg.max_qual = float(A.max_qual); cfg.credit_threshold = A.credit_threshold; cfg.phase_threshold = A.phase_threshold;
    cfg.band_mode = 1;
    for (KmerFamily &F : kmer) kmer_pass(F, cfg, fa);
    vpr_handle *h = nullptr;
    if (vpr_create(&cfg, &h)) { fprintf(stderr, "vpr_create: %s\n", vpr_last_error(nullptr)); return 2; }

    std::vector<ContigOut *> outs;
    for (const std::string &ctg : contigs) {
        const int fi = find(fn, ctg);
        if (fi < 0) die("ERROR: contig '%s' not in reference FASTA", ctg.c_str());
        const uint8_t *seq = fa->seq + fa->ctg_off[fi];
        const int64_t seq_len = fa->ctg_off[fi + 1] - fa->ctg_off[fi];
        const int qi = find(qn, ctg), ti = find(tn, ctg);
        ContigOut *C = new ContigOut();
        C->name = ctg;
        C->slot[0] = qi >= 0 ? &q->vars[2 * qi] : &EMPTY_HAP; C->slot[1] = qi >= 0 ? &q->vars[2 * qi + 1] : &EMPTY_HAP;
        C->slot[2] = ti >= 0 ? &t->vars[2 * ti] : &EMPTY_HAP; C->slot[3] = ti >= 0 ? &t->vars[2 * ti + 1] : &EMPTY_HAP;
        // superclusterData ctor, cluster.cpp:134-157: the query's header wins
        if (qi >= 0) { C->length = q->ctg_len[qi]; C->ploidy = q->ploidy[qi]; }
        else if (ti >= 0) { C->length = t->ctg_len[ti]; C->ploidy = t->ploidy[ti]; }
        else { C->length = seq_len; C->ploidy = 0; }

        // ---- clustering (cluster.cpp:954-1263 on the GPU, or the distance rules) and superclustering (cluster.cpp:404-808)
        vcl_hap haps[4];
        vcl_clusters *cl[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < 4; i++) {
            const vio_hap_vars *s = C->slot[i];
            haps[i] = vcl_hap{s->n, s->pos, s->rlen, s->type, s->ref_len, s->alt_len};
            int rc;
            if (A.cluster == "biwfa") {
                const vcl_hap_seq hs = {haps[i], s->ref_off, s->alt_off, s->pool};
                rc = vcl_wfa_cluster(&hs, seq, int32_t(seq_len), A.sub, A.open, A.extend, A.max_iterations, A.reach_min_gap, A.device, &cl[i], nullptr);
            } else {
                rc = vcl_simple_cluster(&haps[i], A.cluster == "size" ? 1 : 0, A.cluster_gap, A.reach_min_gap, &cl[i]);
            }
            if (rc) die("ERROR: contig '%s': clustering failed (%d)", ctg.c_str(), rc);
        }
        const vcl_clusters *ccl[4] = {cl[0], cl[1], cl[2], cl[3]};
        if (vcl_supercluster(haps, ccl, A.max_supercluster_size, &C->sc)) die("ERROR: contig '%s': superclustering failed", ctg.c_str());
        const vcl_superclusters *sc = C->sc;
        const int n_sc = sc->n;
        std::vector<int64_t> var_off[4];
        for (int i = 0; i < 4; i++) {
            var_off[i].assign(size_t(n_sc) + 1, 0);
            const vcl_clusters *c = sc->clusters[i];
            if (c->n > 0) for (int k = 0; k <= n_sc; k++) var_off[i][size_t(k)] = c->var_beg[sc->brk[i][k]];
        }
        memset(&C->res, 0, sizeof(C->res));
        int n_clusters = 0;
        int64_t n_hapvars = 0;
        for (int i = 0; i < 4; i++) { n_clusters += cl[i]->n; n_hapvars += C->slot[i]->n; }
        if (n_sc > 0) {
            // ---- the path: variant tables + contig over the link, generate_ptrs_strs and everything behind it on the device
            const int64_t ctg_off[2] = {0, seq_len};
            std::vector<int32_t> sc_ctg(size_t(n_sc), 0);
            vpr_variants V;
            memset(&V, 0, sizeof(V));
            V.n_sc = n_sc; V.n_ctg = 1; V.ctg_off = ctg_off; V.ctg_seq = seq; V.sc_ctg = sc_ctg.data(); V.sc_beg = sc->beg; V.sc_end = sc->end;
            static const uint8_t no_pool[1] = {0};
            for (int i = 0; i < 4; i++) {
                const vio_hap_vars *s = C->slot[i];
                V.var_off[i] = var_off[i].data(); V.var_pos[i] = s->pos; V.var_type[i] = s->type; V.var_qual[i] = s->var_qual;
                V.var_ref_off[i] = s->ref_off; V.var_ref_len[i] = s->ref_len; V.var_alt_off[i] = s->alt_off; V.var_alt_len[i] = s->alt_len;
                V.allele_pool[i] = s->pool ? s->pool : no_pool;
            }
            if (vpr_upload_variants(h, &V) || vpr_execute(h)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
            if (vpr_results_alloc(h, &C->res, &C->res_block) || vpr_download(h, &C->res)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
            if (A.distance) {      // edits_wrapper for this contig's superclusters, behind the precision/recall path (main.cpp:223-238)
                vpr_dist_config dc;
                memset(&dc, 0, sizeof(dc));
                dc.eval_sub = A.eval_sub; dc.eval_open = A.eval_open; dc.eval_extend = A.eval_extend; dc.min_qual = A.min_qual; dc.max_qual = A.max_qual;
                vpr_dist_info di;
                if (vpr_distance(h, &V, &dc) || vpr_distance_info(h, &di)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                const size_t ne = size_t(di.n_edits);
                C->e_sc.resize(ne); C->e_pos.resize(ne); C->e_len.resize(ne); C->e_minq.resize(ne); C->e_maxq.resize(ne); C->e_hap.resize(ne); C->e_type.resize(ne);
                std::vector<int64_t> qd(size_t(A.max_qual) + 2);
                vpr_dist_results dr;
                memset(&dr, 0, sizeof(dr));
                dr.qual_dists = qd.data(); dr.edit_sc = C->e_sc.data(); dr.edit_hap = C->e_hap.data(); dr.edit_pos = C->e_pos.data();
                dr.edit_type = C->e_type.data(); dr.edit_len = C->e_len.data(); dr.edit_min_qual = C->e_minq.data(); dr.edit_max_qual = C->e_maxq.data();
                if (vpr_distance_download(h, &dr)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                if (di.n_limit || di.n_error)
                    fprintf(stderr, "[WARN  vcfdist_amd] contig '%s': %lld distance alignment(s) beyond the device's memory plan and %lld that failed: "
                                    "NOT EVALUATED -- left out of the distance metrics\n", ctg.c_str(), (long long)di.n_limit, (long long)di.n_error);
                fprintf(stderr, "[vcfdist_amd] %s: %lld distance alignments, %lld edits, edit distance %lld\n", ctg.c_str(), (long long)di.n_jobs,
                        (long long)di.n_edits, (long long)*std::min_element(qd.begin(), qd.end()));
            }
            // a supercluster with an alignment the GPU path did not evaluate takes no side in the contig's phasing
            const uint32_t err_bits = VPR_ST_ERR_LIMIT | VPR_ST_ERR_NO_PTR | VPR_ST_ERR_UNFINISHED;
            for (int a = 0; a < 4 * n_sc; a++) if (C->res.aln_status[a] & err_bits) C->res.sc_phase[a >> 2] = VPR_PHASE_NONE;
            C->phase_sets = transfer_phase_sets(C->slot, var_off, n_sc);
            C->pb.assign(size_t(n_sc), 0); C->sw.assign(size_t(n_sc), 0); C->fl.assign(size_t(n_sc), 0);
            int32_t ns = 0, nf = 0;
            if (vpr_phase(C->res.sc_phase, C->phase_sets.data(), n_sc, C->pb.data(), C->sw.data(), &ns, C->fl.data(), &nf))
                die("ERROR: contig '%s': unexpected phase", ctg.c_str());
            C->sw.resize(size_t(ns)); C->fl.resize(size_t(nf));
            std::vector<uint8_t> cls[4];
            const uint8_t *clsp[4];
            for (int i = 0; i < 4; i++) {
                const vio_hap_vars *s = C->slot[i];
                cls[i].assign(size_t(std::max(s->n, 1)), 0);
                if (s->n) vpr_var_class(s->type, s->ref_len, s->alt_len, s->n, A.sv_threshold, cls[i].data());
                clsp[i] = cls[i].data();
            }
            std::vector<int64_t> counts(total.size(), 0);
            if (vpr_pr_counts(h, clsp, C->pb.data(), A.min_qual, A.max_qual, counts.data())) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
            for (size_t k = 0; k < total.size(); k++) total[k] += counts[k];
            // the same evaluation, its FP and FN cut by why they are wrong, its TP by how they were matched (the classes are resident)
            auto label = [&](LabelPass &P, auto call) {
                std::vector<int64_t> c(P.total.size(), 0);
                double ms = 0;
                if (call(c.data()) || P.timing(h, &ms)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                for (size_t k = 0; k < c.size(); k++) P.total[k] += c[k];
                P.ms += ms;
            };
            if (A.classify_errors) label(ec, [&](int64_t *c) { return vpr_errclass(h, &V, nullptr, C->pb.data(), A.error_window, A.min_qual, A.max_qual, c); });
            if (A.classify_matches) label(mk, [&](int64_t *c) { return vpr_matchkind(h, &V, nullptr, C->pb.data(), A.min_qual, A.max_qual, c); });
            if (n_strata) {        // the same evaluation, cut by region: membership words, then the histogram per stratum
                std::vector<int64_t> iv_off(size_t(n_bed) + 1, 0);
                std::vector<int32_t> iv_start, iv_stop;
                for (int k = 0; k < n_list; k++) {
                    int64_t n = 0;
                    const int32_t *st = nullptr, *sp = nullptr;
                    if (vio_bed_intervals(strata.beds[size_t(k)], ctg.c_str(), &n, &st, &sp)) die("ERROR: %s", vio_last_error());
                    iv_start.insert(iv_start.end(), st, st + n); iv_stop.insert(iv_stop.end(), sp, sp + n);
                    iv_off[size_t(k) + 1] = int64_t(iv_start.size());
                }
                size_t row = size_t(n_list);
                for (const KmerFamily &F : kmer)       // the contig's rows of the repeat strata, then of the long ones, as ordinary BED rows behind the list's
                    for (int k = 0; k < F.n; k++) {
                        const size_t r = size_t(k) * size_t(fa->n_ctg) + size_t(fi);
                        iv_start.insert(iv_start.end(), F.start.begin() + F.off[r], F.start.begin() + F.off[r + 1]);
                        iv_stop.insert(iv_stop.end(), F.stop.begin() + F.off[r], F.stop.begin() + F.off[r + 1]);
                        iv_off[++row] = int64_t(iv_start.size());
                    }
                const vpr_strata ST = {n_bed, 1, iv_off.data(), iv_start.data(), iv_stop.data()};
                std::vector<int64_t> sc_counts(strat_total.size(), 0);
                // (with --stratify-context the context intervals are built on the device and go to the same mask kernel)
                if (n_pre && (n_ctx ? vpr_context_masks(h, &V, n_bed ? &ST : nullptr, ctx_spec, n_ctx) : vpr_strata_masks(h, &V, &ST)))
                    die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                // (with --stratify-variants the bits made from the variant tables follow in the same words)
                if (n_vs) {
                    double ms = 0;
                    if (vpr_varstrata_masks(h, &V, vs_spec, n_vs, n_pre ? 1 : 0) || vpr_varstrata_timing(h, &ms)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                    vs_ms += ms;
                }
                if (vpr_pr_counts_strata(h, nullptr, C->pb.data(), A.min_qual, A.max_qual, sc_counts.data()))
                    die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                for (size_t k = 0; k < strat_total.size(); k++) strat_total[k] += sc_counts[k];
                const size_t n_words = (size_t(n_strata) + 63) / 64;
                std::vector<uint64_t> words[4];
                uint64_t *wp[4];
                for (int i = 0; i < 4; i++) { words[i].assign(std::max<size_t>(n_words * size_t(C->slot[i]->n), 1), 0); wp[i] = words[i].data(); }
                if (vpr_strata_download_masks(h, wp)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                if (n_ctx) keep_context_intervals(h, ctg);
                for (int i = 0; i < 4; i++) {
                    const size_t nv = size_t(C->slot[i]->n);
                    for (size_t v = 0; v < nv; v++) {
                        uint64_t any = 0;
                        for (size_t w = 0; w < n_words; w++) any |= words[i][w * nv + v];
                        strat_none += any == 0;
                        for (int k = 0; k < n_vs; k++)
                            (i < 2 ? vs_query : vs_truth)[size_t(k)] += int64_t(words[i][size_t((n_pre + k) >> 6) * nv + v] >> ((n_pre + k) & 63) & 1);
                    }
                    strat_vars += int64_t(nv);
                }
            }
            if (A.bootstrap) {     // the same evaluation, resampled over superclusters (after the masks: a pass per stratum cuts by them)
                const size_t ordinal = size_t(&ctg - contigs.data());
                std::vector<uint64_t> keys(static_cast<size_t>(n_sc), 0);
                for (int k = 0; k < n_sc; k++) keys[size_t(k)] = (uint64_t(ordinal) << 32) | uint64_t(k);
                std::vector<int64_t> rep(boot_total.size(), 0);
                for (int k = -1; k < n_strata; k++) {
                    int32_t grid[3];
                    double ms = 0;
                    if (vpr_pr_counts_boot(h, nullptr, C->pb.data(), A.min_qual, A.max_qual, keys.data(), A.bootstrap_seed, A.bootstrap, k, rep.data()) ||
                        vpr_boot_info(h, grid, &ms))
                        die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                    int64_t *into = k < 0 ? boot_total.data() : boot_strat.data() + size_t(k) * rep.size();
                    for (size_t j = 0; j < rep.size(); j++) into[j] += rep[j];
                    boot_ms += ms;
                }
            }
            if (A.cut_classes) {   // the labels of the same evaluation cut and resampled: their bytes and the words are both resident now
                const size_t ordinal = size_t(&ctg - contigs.data());
                std::vector<uint64_t> keys(static_cast<size_t>(n_sc), 0);
                for (int k = 0; k < n_sc; k++) keys[size_t(k)] = (uint64_t(ordinal) << 32) | uint64_t(k);
                for (LabelPass *P : {&ec, &mk}) {
                    if (P->total.empty()) continue;
                    double ms_strata = 0, ms_boot = 0;
                    std::vector<int64_t> c(std::max(P->strata.size(), P->boot.size()), 0);
                    if (n_strata) {
                        if (P->cut_strata(h, A.min_qual, A.max_qual, c.data()) || P->cut_timing(h, &ms_strata, &ms_boot))
                            die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                        for (size_t k = 0; k < P->strata.size(); k++) P->strata[k] += c[k];
                        P->cut_ms += ms_strata;
                    }
                    if (A.bootstrap) {
                        if (P->cut_boot(h, A.min_qual, A.max_qual, keys.data(), A.bootstrap_seed, A.bootstrap, -1, c.data()) ||
                            P->cut_timing(h, &ms_strata, &ms_boot))
                            die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                        for (size_t k = 0; k < P->boot.size(); k++) P->boot[k] += c[k];
                        P->cut_ms += ms_boot;
                    }
                }
            }
            // the reference's WARN lines (dist.cpp:1203-1223) and -- loudly -- what this implementation did not evaluate
            static const struct { uint32_t bit; const char *text; } W[] = {
                {VPR_ST_WARN_REF_ED, "Nonzero reference edit distance with no truth variants at ctg %s supercluster %d"},
                {VPR_ST_WARN_QUERY_ED, "Query edit distance changed with no query variants at ctg %s supercluster %d"},
                {VPR_ST_WARN_EXCEEDS, "Query edit distance exceeds reference edit distance at ctg %s supercluster %d"},
                {VPR_ST_WARN_ZERO_ED, "Zero edit distance with truth variants at ctg %s supercluster %d"}};
            for (const auto &w : W)
                for (int a = 0; a < 4 * n_sc; a++)
                    if (C->res.aln_status[a] & w.bit) { fputs("[WARN  vcfdist] ", stderr); fprintf(stderr, w.text, ctg.c_str(), a / 4); fputc('\n', stderr); }
            int n_bad = 0;
            for (int k = 0; k < n_sc; k++) {
                bool bad = false;
                for (int i = 0; i < 4; i++) bad = bad || (C->res.aln_status[4 * k + i] & err_bits);
                n_bad += bad;
            }
            if (n_bad) {
                fprintf(stderr, "[WARN  vcfdist_amd] contig '%s': %d supercluster(s) with alignments beyond an implementation limit of the GPU path: "
                                "NOT EVALUATED -- their variants are left out of every count and table\n", ctg.c_str(), n_bad);
                if (A.strict) die("ERROR: contig '%s': %d supercluster(s) not evaluated (--strict)", ctg.c_str(), n_bad);
            }
        } else {
            // (no superclusters: the writers still want the per-variant columns -- there are no variants either)
            static uint8_t zero8[1]; static int32_t zero32[1]; static float zerof[1];
            for (int i = 0; i < 4; i++)
                for (int w = 0; w < 2; w++) {
                    C->res.errtype[i][w] = zero8; C->res.sync_group[i][w] = zero32; C->res.credit[i][w] = zerof;
                    C->res.ref_ed[i][w] = zero32; C->res.query_ed[i][w] = zero32; C->res.callq[i][w] = zerof;
                }
            C->res.sc_phase = zero32; C->res.orig_phase_dist = zero32; C->res.swap_phase_dist = zero32;
            if (n_ctx) {           // context-strata.bed lists every evaluated contig: the intervals alone, for no variant
                const int64_t ctg_off[2] = {0, seq_len}, none[1] = {0};
                vpr_variants V;
                memset(&V, 0, sizeof(V));
                V.n_ctg = 1; V.ctg_off = ctg_off; V.ctg_seq = seq;
                for (int i = 0; i < 4; i++) V.var_off[i] = none;
                if (vpr_context_masks(h, &V, nullptr, ctx_spec, n_ctx)) die("ERROR: contig '%s': %s", ctg.c_str(), vpr_last_error(h));
                keep_context_intervals(h, ctg);
            }
        }
        fprintf(stderr, "[vcfdist_amd] %s: %lld hap-variants, %d clusters, %d superclusters, %zu switch / %zu flip errors\n", ctg.c_str(),
                (long long)n_hapvars, n_clusters, n_sc, C->sw.size(), C->fl.size());
        C->phase_block.assign(size_t(n_sc) + 1, 0);
        const int32_t n_pb = vrp_phase_blocks(C->phase_sets.data(), n_sc, C->phase_block.data());
        C->phase_block.resize(size_t(std::max(n_pb, 0)) + 1);
        for (int i = 0; i < 4; i++) vcl_clusters_free(cl[i]);
        outs.push_back(C);
    }

    if (A.distance) {      // write_distance (printed even with -n), write_edits (edit.cpp:134-280)
        std::vector<vrp_edits> sets(outs.size());
        for (size_t k = 0; k < outs.size(); k++) {
            const ContigOut *C = outs[k];
            sets[k] = vrp_edits{C->name.c_str(), int64_t(C->e_sc.size()), C->e_sc.data(), C->e_hap.data(), C->e_pos.data(), C->e_type.data(),
                                C->e_len.data(), C->e_minq.data(), C->e_maxq.data()};
        }
        std::vector<char> text(size_t(1) << 16);
        const int n = vrp_write_distance(A.prefix.c_str(), sets.data(), int32_t(sets.size()), A.min_qual, A.max_qual, A.eval_sub, A.eval_open,
                                         A.eval_extend, 1, A.no_output_files ? 0 : 1, text.data(), int64_t(text.size()));
        if (n < 0) die("ERROR: %s", vrp_last_error());
        if (!A.no_output_files && vrp_write_edits((A.prefix + "edits.tsv").c_str(), sets.data(), int32_t(sets.size())))
            die("ERROR: %s", vrp_last_error());
        printf("%s\n", text.data());
    }
    vpr_pr_row rows[2 * VPR_VARTYPES];
    if (vpr_pr_summary(total.data(), A.min_qual, A.max_qual, rows)) die("ERROR: vpr_pr_summary failed");
    if (!A.no_output_files) {
        if (vrp_write_precision_recall(A.prefix.c_str(), total.data(), A.min_qual, A.max_qual)) die("ERROR: %s", vrp_last_error());
        write_params(A, cmd);
        if (n_strata) {
            std::vector<const char *> names;
            for (const auto &n : strata.names) names.push_back(n.c_str());
            if (vrp_write_stratified(A.prefix.c_str(), names.data(), n_strata, strat_total.data(), A.min_qual, A.max_qual)) die("ERROR: %s", vrp_last_error());
            if (A.bootstrap && vrp_write_bootstrap_stratified(A.prefix.c_str(), names.data(), n_strata, strat_total.data(), boot_strat.data(), A.bootstrap,
                                                              A.bootstrap_seed, A.min_qual, A.max_qual))
                die("ERROR: %s", vrp_last_error());
            // repeat-strata.bed and long-repeat-strata.bed: the evaluated contigs in evaluation order, rows contig-major
            for (const KmerFamily &F : kmer) {
                if (!F.n) continue;
                std::vector<const char *> cn;
                std::vector<int64_t> off(1, 0);
                std::vector<int32_t> st, sp;
                for (const auto &c : contigs) {
                    cn.push_back(c.c_str());
                    const int fi = find(fn, c);
                    for (int k = 0; k < F.n; k++) {
                        const size_t r = size_t(k) * size_t(fa->n_ctg) + size_t(fi);
                        st.insert(st.end(), F.start.begin() + F.off[r], F.start.begin() + F.off[r + 1]);
                        sp.insert(sp.end(), F.stop.begin() + F.off[r], F.stop.begin() + F.off[r + 1]);
                        off.push_back(int64_t(st.size()));
                    }
                }
                st.push_back(0); sp.push_back(0);      // (never empty: a pointer is wanted)
                if (F.write_bed(A.prefix.c_str(), cn.data(), int32_t(cn.size()), F.names, F.n, off.data(), st.data(), sp.data())) die("ERROR: %s", vrp_last_error());
            }
            if (n_ctx) {
                std::vector<const char *> cn;
                for (const auto &c : ctx_contigs) cn.push_back(c.c_str());
                if (vrp_write_context_bed(A.prefix.c_str(), cn.data(), int32_t(cn.size()), ctx_names, n_ctx, ctx_off.data(), ctx_start.data(), ctx_stop.data()))
                    die("ERROR: %s", vrp_last_error());
            }
            if (n_vs && vrp_write_variant_strata(A.prefix.c_str(), vs_names, vs_spec, n_vs, vs_query.data(), vs_truth.data())) die("ERROR: %s", vrp_last_error());
        }
        for (const LabelPass *P : {&ec, &mk})
            if (!P->total.empty() && P->write(A.prefix.c_str(), P->total.data(), total.data(), A.min_qual, A.max_qual)) die("ERROR: %s", vrp_last_error());
        if (A.bootstrap && vrp_write_bootstrap(A.prefix.c_str(), total.data(), boot_total.data(), A.bootstrap, A.bootstrap_seed, A.min_qual, A.max_qual))
            die("ERROR: %s", vrp_last_error());
        if (A.cut_classes) {
            std::vector<const char *> names;
            for (const auto &n : strata.names) names.push_back(n.c_str());
            for (const LabelPass *P : {&ec, &mk}) {
                if (P->total.empty()) continue;
                if (n_strata && P->write_strata(A.prefix.c_str(), names.data(), n_strata, P->strata.data(), strat_total.data(), A.min_qual, A.max_qual))
                    die("ERROR: %s", vrp_last_error());
                if (A.bootstrap && P->write_boot(A.prefix.c_str(), P->total.data(), total.data(), P->boot.data(), A.bootstrap, A.min_qual, A.max_qual))
                    die("ERROR: %s", vrp_last_error());
            }
        }
        std::vector<vrp_contig> ctgs(outs.size());
        for (size_t k = 0; k < outs.size(); k++) {
            ContigOut *C = outs[k];
            vrp_contig &c = ctgs[k];
            memset(&c, 0, sizeof(c));
            const int fi = find(fn, C->name);
            c.name = C->name.c_str(); c.length = int32_t(C->length); c.ploidy = C->ploidy;
            c.seq = fa->seq + fa->ctg_off[fi]; c.seq_len = fa->ctg_off[fi + 1] - fa->ctg_off[fi];
            static const uint8_t no_pool[1] = {0};
            for (int i = 0; i < 4; i++) {
                const vio_hap_vars *s = C->slot[i];
                vrp_hap &hp = c.hap[i];
                hp.n_var = s->n; hp.pos = s->pos; hp.type = s->type; hp.loc = nullptr; hp.var_qual = s->var_qual; hp.phase_set = s->phase_set;
                hp.ref_len = s->ref_len; hp.alt_len = s->alt_len; hp.ref_off = s->ref_off; hp.alt_off = s->alt_off; hp.pool = s->pool ? s->pool : no_pool;
                hp.n_cluster = C->sc->clusters[i]->n;
                hp.cluster_beg = C->sc->clusters[i]->n ? C->sc->clusters[i]->var_beg : nullptr;
                for (int w = 0; w < 2; w++) {
                    hp.errtype[w] = C->res.errtype[i][w]; hp.credit[w] = C->res.credit[i][w]; hp.sync_group[w] = C->res.sync_group[i][w];
                    hp.ref_ed[w] = C->res.ref_ed[i][w]; hp.query_ed[w] = C->res.query_ed[i][w];
                }
                c.sc_brk[i] = C->sc->brk[i];
            }
            c.n_sc = C->sc->n; c.sc_beg = C->sc->beg; c.sc_end = C->sc->end;
            c.sc_phase = C->res.sc_phase; c.pb_phase = C->pb.data(); c.orig_phase_dist = C->res.orig_phase_dist; c.swap_phase_dist = C->res.swap_phase_dist;
            c.sc_phase_set = C->phase_sets.data(); c.n_pb = int32_t(C->phase_block.size()) - 1; c.phase_block = C->phase_block.data();
            c.n_switches = int32_t(C->sw.size()); c.n_flips = int32_t(C->fl.size()); c.switches = C->sw.data(); c.flips = C->fl.data();
        }
        const int32_t n = int32_t(ctgs.size());
        auto path = [&](const char *name) { return A.prefix + name; };
        if (vrp_write_phase_blocks(path("phase-blocks.tsv").c_str(), ctgs.data(), n) || vrp_write_switchflips(path("switchflips.tsv").c_str(), ctgs.data(), n) ||
            vrp_write_phasing_summary(path("phasing-summary.tsv").c_str(), ctgs.data(), n) || vrp_write_superclusters(path("superclusters.tsv").c_str(), ctgs.data(), n) ||
            vrp_write_variants(path("query.tsv").c_str(), ctgs.data(), n, 0) || vrp_write_variants(path("truth.tsv").c_str(), ctgs.data(), n, 1) ||
            vrp_write_summary_vcf(path("summary.vcf").c_str(), ctgs.data(), n, cmd.c_str(), nullptr, float(A.credit_threshold)))
            die("ERROR: %s", vrp_last_error());
        if (A.realign_query) write_callset_vcf(A.prefix + "query.vcf", q, fa, fn);
        if (A.realign_truth) write_callset_vcf(A.prefix + "truth.vcf", t, fa, fn);
    }
    if (n_strata)
        fprintf(stderr, "[vcfdist_amd] stratified: %d strata, %lld of %lld hap-variants in none of them\n", n_strata, (long long)strat_none,
                (long long)strat_vars);
    for (const KmerFamily &F : kmer) kmer_report(F);
    if (n_ctx)
        fprintf(stderr, "[vcfdist_amd] context strata: %lld intervals of %d strata, %.3f ms on the device\n", (long long)ctx_start.size(), n_ctx, ctx_ms);
    if (n_vs)
        fprintf(stderr, "[vcfdist_amd] variant strata: %d strata, %.3f ms on the device\n", n_vs, vs_ms);
    if (A.classify_errors) {      // the classified errors at threshold NONE: the ALL rows' classes of both callsets
        const size_t nq = size_t(A.max_qual - A.min_qual + 1);
        long long n_fp = 0, n_fn = 0;
        for (int c = 0; c < VPR_EC_CLASSES; c++) {
            n_fp += ec.total[((size_t(0) * VPR_VARTYPES + VPR_VARTYPE_ALL) * VPR_EC_CLASSES + size_t(c)) * nq];
            n_fn += ec.total[((size_t(1) * VPR_VARTYPES + VPR_VARTYPE_ALL) * VPR_EC_CLASSES + size_t(c)) * nq];
        }
        fprintf(stderr, "[vcfdist_amd] error classes: window %d, %lld query FP and %lld truth FN classified, %.3f ms on the device\n", A.error_window,
                n_fp, n_fn, ec.ms);
    }
    if (A.classify_matches) {     // the matched variants at threshold NONE: the ALL rows' kinds of both callsets
        const size_t nq = size_t(A.max_qual - A.min_qual + 1);
        long long n[2][VPR_MK_KINDS];
        for (int cs = 0; cs < 2; cs++)
            for (int c = 0; c < VPR_MK_KINDS; c++) n[cs][c] = mk.total[((size_t(cs) * VPR_VARTYPES + VPR_VARTYPE_ALL) * VPR_MK_KINDS + size_t(c)) * nq];
        fprintf(stderr, "[vcfdist_amd] match kinds: query TP %lld exact, %lld shifted, %lld regrouped, %lld partial; truth TP %lld exact, %lld shifted, "
                "%lld regrouped, %lld partial, %.3f ms on the device\n", n[0][0], n[0][1], n[0][2], n[0][3], n[1][0], n[1][1], n[1][2], n[1][3], mk.ms);
    }
    if (A.cut_classes)
        for (const LabelPass *P : {&ec, &mk}) {
            if (P->total.empty()) continue;
            std::string what;
            if (n_strata) what += std::to_string(n_strata) + " strata, ";
            if (A.bootstrap) what += std::to_string(A.bootstrap) + " replicates, ";
            fprintf(stderr, "[vcfdist_amd] %s cut: %s%.3f ms on the device\n", P->noun, what.c_str(), P->cut_ms);
        }
    if (A.bootstrap)
        fprintf(stderr, "[vcfdist_amd] bootstrap: %d replicates, seed %llu, %.3f ms on the device\n", A.bootstrap, (unsigned long long)A.bootstrap_seed, boot_ms);
    printf("PRECISION-RECALL SUMMARY\n\n");
    printf("TYPE\tTHRESHOLD\tTRUTH_TP\tQUERY_TP\tTRUTH_FN\tQUERY_FP\tPREC\t\tRECALL\t\tF1_SCORE\tF1_QSCORE\n");
    static const char *NAMES[] = {"SNP", "INDEL", "SV", "ALL"};
    for (const vpr_pr_row &r : rows) {
        printf("%s\t%s Q >= %-2d\t%-16d%-16d%-16d%-16d%f\t%f\t%f\t%f\n", NAMES[r.vartype], r.best ? "BEST" : "NONE", r.qual, r.truth_tp, r.query_tp,
               r.truth_fn, r.query_fp, r.precision, r.recall, r.f1_score, r.f1_qscore);
        if (r.best) printf("\n");
    }
    for (ContigOut *C : outs) {
        if (C->res_block) vpr_host_free(C->res_block);
        vcl_superclusters_free(C->sc);
        delete C;
    }
    vpr_destroy(h);
    release_realigned();
    vio_callset_free(q); vio_callset_free(t); vio_fasta_free(fa);
    if (bed) vio_bed_free(bed);
    for (vio_bed *b : strata.beds) vio_bed_free(b);
    return 0;
}
