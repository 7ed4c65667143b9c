// ref_harness.cpp -- drives vcfdist's own functions from flat case files (test infrastructure only).
//
// Linked against the reference's translation units, compiled unmodified from where they lie (oracle/Makefile, target
// `ref`), and against oracle/ref_shim (a stand-in for the twelve htslib calls the reference's VCF reader makes: the
// harness never reads a VCF, it fills the reference's structures through their public members).  Everything below is
// ours; nothing of the reference is restated here -- the functions under test are called, in main.cpp's order.
//
//   ref_harness <subcommand> <case file> <result file>
//
// One case per process: the reference's ERROR() calls exit(1), which the caller sees as a refusal.  Results go to a
// file because the reference prints INFO lines even at verbosity 0.
//
// Case and result files hold data only, as a sequence of named records:
//   I <name> <n>\n<n decimal integers separated by blanks>\n        (floats travel as their 32-bit patterns)
//   S <name> <n>\n<n raw bytes>\n
//
// Subcommands (tests/ref_pins.py writes the cases and documents every record):
//   swg      pairs of strings + penalties -> wf_swg_align score, wf_swg_backtrack CIGAR, count_dist, on reversed strings
//            with the CIGAR reversed back, exactly as edits_wrapper and wf_swg_realign call them
//   ed       pairs of strings -> wf_ed score
//   cluster  variant tables -> simple_cluster / wf_swg_cluster cluster starts and reaches (as `chain`, stopping there)
//   chain    four haplotypes' variant tables + contigs + options -> main.cpp's sequence from check_contigs on
//   realign  the query callset's variant tables -> clustering, wf_swg_realign, left_shift: every column
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "variant.h"
#include "print.h"
#include "globals.h"
#include "fasta.h"
#include "bed.h"
#include "dist.h"
#include "cluster.h"
#include "phase.h"
#include "timer.h"

extern std::vector<std::string> timer_strs;     // defined by the reference's main.cpp, like `g` and the other tables

namespace {

struct Records {
    std::map<std::string, std::vector<int64_t>> ints;
    std::map<std::string, std::string> strs;
    std::vector<std::string> order;

    void read(const char *path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) { fprintf(stderr, "ref_harness: cannot open case '%s'\n", path); exit(2); }
        std::string kind, name;
        long long n;
        while (f >> kind >> name >> n) {
            if (kind == "I") {
                std::vector<int64_t> &v = ints[name];
                v.resize(size_t(n));
                for (long long k = 0; k < n; k++) { long long x; f >> x; v[size_t(k)] = x; }
            } else if (kind == "S") {
                f.get();                        // the newline after the header
                std::string &s = strs[name];
                s.resize(size_t(n));
                if (n) f.read(&s[0], n);
            } else { fprintf(stderr, "ref_harness: bad record kind '%s'\n", kind.data()); exit(2); }
            if (!f) { fprintf(stderr, "ref_harness: truncated record '%s'\n", name.data()); exit(2); }
        }
    }
    const std::vector<int64_t> &I(const std::string &name) const {
        auto it = ints.find(name);
        if (it == ints.end()) { fprintf(stderr, "ref_harness: case lacks '%s'\n", name.data()); exit(2); }
        return it->second;
    }
    const std::string &S(const std::string &name) const {
        auto it = strs.find(name);
        if (it == strs.end()) { fprintf(stderr, "ref_harness: case lacks '%s'\n", name.data()); exit(2); }
        return it->second;
    }
    bool has(const std::string &name) const { return ints.count(name) || strs.count(name); }

    template <typename T> void put(const std::string &name, const std::vector<T> &v) {
        std::vector<int64_t> &d = ints[name];
        if (d.empty() && !std::count(order.begin(), order.end(), name)) order.push_back(name);
        for (const T &x : v) d.push_back(int64_t(x));
    }
    void put1(const std::string &name, int64_t x) { put(name, std::vector<int64_t>{x}); }
    void touch(const std::string &name) { put(name, std::vector<int64_t>{}); }
    void put_bits(const std::string &name, const std::vector<float> &v) {
        std::vector<int64_t> b;
        for (float x : v) { uint32_t u; std::memcpy(&u, &x, 4); b.push_back(u); }
        put(name, b);
    }
    void write(const char *path) const {
        FILE *f = fopen(path, "wb");
        if (!f) { fprintf(stderr, "ref_harness: cannot write '%s'\n", path); exit(2); }
        for (const std::string &name : order) {
            const std::vector<int64_t> &v = ints.at(name);
            fprintf(f, "I %s %zu\n", name.data(), v.size());
            for (size_t k = 0; k < v.size(); k++) fprintf(f, k ? " %lld" : "%lld", (long long)v[k]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
};

std::vector<std::string> split_lines(const std::string &s) {
    std::vector<std::string> out;
    size_t a = 0;
    while (a < s.size()) {
        size_t b = s.find('\n', a);
        if (b == std::string::npos) b = s.size();
        out.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return out;
}

std::string piece(const std::string &pool, const std::vector<int64_t> &off, size_t k) {
    return pool.substr(size_t(off[k]), size_t(off[k + 1] - off[k]));
}

// ---- swg / ed: function level ------------------------------------------------------------------------------------

int run_swg(const Records &in, Records &out) {
    const std::vector<int64_t> &pen = in.I("pen"), &qo = in.I("q_off"), &to = in.I("t_off");
    const std::string &qs = in.S("q"), &ts = in.S("t");
    out.touch("score"); out.touch("dist"); out.touch("cigar_off"); out.touch("cigar");
    out.put1("cigar_off", 0);
    int64_t total = 0;
    for (size_t k = 0; k + 1 < qo.size(); k++) {
        std::string query = piece(qs, qo, k), truth = piece(ts, to, k);
        std::vector< std::vector< std::vector<uint8_t> > > ptrs(MATS);
        std::vector< std::vector< std::vector<int> > > offs(MATS);
        int s = 0;
        std::reverse(query.begin(), query.end());
        std::reverse(truth.begin(), truth.end());
        wf_swg_align(query, truth, ptrs, offs, s, int(pen[0]), int(pen[1]), int(pen[2]), false);
        std::vector<int> cigar = wf_swg_backtrack(query, truth, ptrs, offs, s, int(pen[0]), int(pen[1]), int(pen[2]), false);
        std::reverse(cigar.begin(), cigar.end());
        out.put1("score", s);
        out.put1("dist", count_dist(cigar));
        out.put("cigar", cigar);
        total += int64_t(cigar.size());
        out.put1("cigar_off", total);
    }
    return 0;
}

int run_ed(const Records &in, Records &out) {
    const std::vector<int64_t> &qo = in.I("q_off"), &to = in.I("t_off");
    const std::string &qs = in.S("q"), &ts = in.S("t");
    out.touch("score");
    for (size_t k = 0; k + 1 < qo.size(); k++) {
        std::vector< std::vector<int> > offs, ptrs;
        int s = 0;
        wf_ed(piece(qs, qo, k), piece(ts, to, k), s, offs, ptrs, false);
        out.put1("score", s);
    }
    return 0;
}

// ---- the chain ---------------------------------------------------------------------------------------------------

struct Case {
    std::vector<std::string> ctg_names;
    std::shared_ptr<fastaData> ref;
    std::shared_ptr<variantData> callset[2];
};

void parse_globals(const Records &in, const char *case_path) {
    // argv: program, query.vcf, truth.vcf (never opened: ref_shim), ref.fa (only opened: any readable file), options
    std::vector<std::string> args = {"ref_harness", "query.vcf", "truth.vcf", case_path};
    for (const std::string &a : split_lines(in.S("args"))) if (!a.empty()) args.push_back(a);
    std::vector<char *> argv;
    for (std::string &a : args) argv.push_back(&a[0]);
    g.parse_args(int(argv.size()), argv.data());
    g.init_timers(timer_strs);
}

Case build_case(const Records &in) {
    Case c;
    c.ctg_names = split_lines(in.S("ctg_names"));
    const std::vector<int64_t> &co = in.I("ctg_off");
    const std::string &seq = in.S("ctg_seq");
    FILE *none = fopen("/dev/null", "r");
    c.ref.reset(new fastaData(none));            // the stand-in tokeniser reads nothing; the sequences come from the case
    for (size_t k = 0; k < c.ctg_names.size(); k++) {
        c.ref->fasta[c.ctg_names[k]] = seq.substr(size_t(co[k]), size_t(co[k + 1] - co[k]));
        c.ref->lengths[c.ctg_names[k]] = int(co[k + 1] - co[k]);
    }
    for (int cs = 0; cs < 2; cs++) {
        std::shared_ptr<variantData> v(new variantData());
        v->callset = cs;
        v->filename = cs == QUERY ? "query.vcf" : "truth.vcf";
        v->sample = "SAMPLE";
        v->ref = c.ref;
        for (int64_t k : in.I(cs == QUERY ? "query_ctgs" : "truth_ctgs")) {
            const std::string &name = c.ctg_names[size_t(k)];
            v->contigs.push_back(name);
            v->lengths.push_back(c.ref->lengths.at(name));
            v->ploidy.push_back(2);
            for (int hap = 0; hap < HAPS; hap++) v->variants[hap][name] = std::shared_ptr<ctgVariants>(new ctgVariants());
        }
        for (int hap = 0; hap < HAPS; hap++) {
            const std::string p = "v" + std::to_string(cs * 2 + hap) + "_";
            const std::vector<int64_t> &ctg = in.I(p + "ctg"), &pos = in.I(p + "pos"), &rlen = in.I(p + "rlen"), &type = in.I(p + "type"),
                                       &loc = in.I(p + "loc"), &gt = in.I(p + "orig_gt"), &ps = in.I(p + "phase_set"), &vq = in.I(p + "var_qual"),
                                       &gq = in.I(p + "gt_qual"), &ro = in.I(p + "ref_off"), &ao = in.I(p + "alt_off");
            const std::string &refs = in.S(p + "refs"), &alts = in.S(p + "alts");
            for (size_t k = 0; k < pos.size(); k++) {
                const std::string &name = c.ctg_names[size_t(ctg[k])];
                if (!v->variants[hap].count(name)) { fprintf(stderr, "ref_harness: variant on a contig its callset lacks\n"); exit(2); }
                float fv, fg;
                uint32_t uv = uint32_t(vq[k]), ug = uint32_t(gq[k]);
                std::memcpy(&fv, &uv, 4); std::memcpy(&fg, &ug, 4);
                v->variants[hap][name]->add_var(int(pos[k]), int(rlen[k]), uint8_t(hap), uint8_t(type[k]), uint8_t(loc[k]),
                                                piece(refs, ro, k), piece(alts, ao, k), uint8_t(gt[k]), fg, fv, int(ps[k]));
            }
        }
        c.callset[cs] = v;
    }
    return c;
}

// main.cpp's clustering step for one callset
void cluster_callset(std::shared_ptr<variantData> v, int callset) {
    if (g.cluster_method == "gap" || g.cluster_method == "size") {
        simple_cluster(v, callset);
    } else if (g.cluster_method == "biwfa") {
        // every (contig, hap) is clustered on its own: one after the other here, the reference spreads them over threads
        for (int ctg = 0; ctg < int(v->contigs.size()); ctg++)
            for (int hap = 0; hap < HAPS; hap++) wf_swg_cluster(v.get(), ctg, hap, g.sub, g.open, g.extend);
    } else {
        fprintf(stderr, "ref_harness: clustering method '%s'\n", g.cluster_method.data());
        exit(1);
    }
}

// per hap slot, contigs in the case's order: cluster starts and reaches, with offsets per contig
void put_clusters(const Case &c, Records &out) {
    for (int slot = 0; slot < 4; slot++) {
        const std::string p = "c" + std::to_string(slot) + "_";
        for (const char *f : {"off", "start", "left", "right"}) out.touch(p + f);
        out.put1(p + "off", 0);
        int64_t total = 0;
        for (const std::string &name : c.ctg_names) {
            auto &m = c.callset[slot >> 1]->variants[slot & 1];
            auto it = m.find(name);
            if (it != m.end()) {
                const ctgVariants &v = *it->second;
                out.put(p + "start", v.clusters);
                out.put(p + "left", v.left_reaches);
                out.put(p + "right", v.right_reaches);
                total += int64_t(v.clusters.size());
                if (v.left_reaches.size() != v.clusters.size() || v.right_reaches.size() != v.clusters.size()) {
                    fprintf(stderr, "ref_harness: reaches and clusters differ in length\n"); exit(2);
                }
            }
            out.put1(p + "off", total);
        }
    }
}

void put_variant_columns(const Case &c, int n_slots, Records &out) {
    for (int slot = 0; slot < n_slots; slot++) {
        const std::string p = "r" + std::to_string(slot) + "_";
        for (const char *f : {"off", "pos", "rlen", "type", "loc", "orig_gt", "phase_set", "var_qual", "gt_qual", "ref_len", "alt_len"}) out.touch(p + f);
        std::string refs, alts;
        out.put1(p + "off", 0);
        int64_t total = 0;
        for (const std::string &name : c.ctg_names) {
            auto &m = c.callset[slot >> 1]->variants[slot & 1];
            auto it = m.find(name);
            if (it != m.end()) {
                const ctgVariants &v = *it->second;
                out.put(p + "pos", v.poss); out.put(p + "rlen", v.rlens); out.put(p + "type", v.types); out.put(p + "loc", v.locs);
                out.put(p + "orig_gt", v.orig_gts); out.put(p + "phase_set", v.phase_sets);
                out.put_bits(p + "var_qual", v.var_quals); out.put_bits(p + "gt_qual", v.gt_quals);
                for (int k = 0; k < v.n; k++) {
                    out.put1(p + "ref_len", int64_t(v.refs[k].size())); out.put1(p + "alt_len", int64_t(v.alts[k].size()));
                    out.put(p + "refs", std::vector<char>(v.refs[k].begin(), v.refs[k].end()));
                    out.put(p + "alts", std::vector<char>(v.alts[k].begin(), v.alts[k].end()));
                }
                total += v.n;
            }
            out.put1(p + "off", total);
        }
        out.touch(p + "refs"); out.touch(p + "alts");
    }
}

int run_cluster(const Records &in, Records &out, const char *case_path) {
    parse_globals(in, case_path);
    Case c = build_case(in);
    cluster_callset(c.callset[QUERY], QUERY);
    cluster_callset(c.callset[TRUTH], TRUTH);
    put_clusters(c, out);
    return 0;
}

int run_realign(const Records &in, Records &out, const char *case_path) {
    parse_globals(in, case_path);
    Case c = build_case(in);
    cluster_callset(c.callset[QUERY], QUERY);
    put_clusters(c, out);
    c.callset[QUERY] = wf_swg_realign(c.callset[QUERY], c.ref, g.sub, g.open, g.extend, QUERY);
    c.callset[QUERY]->left_shift();
    put_variant_columns(c, 2, out);
    return 0;
}

int run_chain(const Records &in, Records &out, const char *case_path) {
    parse_globals(in, case_path);
    Case c = build_case(in);
    std::shared_ptr<variantData> query_ptr = c.callset[QUERY], truth_ptr = c.callset[TRUTH];
    std::shared_ptr<fastaData> ref_ptr = c.ref;

    // main.cpp from check_contigs on, the reference's own calls in its own order
    check_contigs(query_ptr, truth_ptr, ref_ptr);
    if (g.realign_query) {
        cluster_callset(query_ptr, QUERY);
        query_ptr = wf_swg_realign(query_ptr, ref_ptr, g.sub, g.open, g.extend, QUERY);
        query_ptr->left_shift();
    }
    cluster_callset(query_ptr, QUERY);
    if (g.realign_truth) {
        cluster_callset(truth_ptr, TRUTH);
        truth_ptr = wf_swg_realign(truth_ptr, ref_ptr, g.sub, g.open, g.extend, TRUTH);
        truth_ptr->left_shift();
    }
    cluster_callset(truth_ptr, TRUTH);
    c.callset[QUERY] = query_ptr; c.callset[TRUTH] = truth_ptr;
    put_clusters(c, out);

    std::shared_ptr<superclusterData> clusterdata_ptr(new superclusterData(query_ptr, truth_ptr, ref_ptr));
    auto sc_groups = sort_superclusters(clusterdata_ptr);
    precision_recall_threads_wrapper(clusterdata_ptr, sc_groups);
    editData edits;
    if (g.distance) edits = edits_wrapper(clusterdata_ptr);
    std::unique_ptr<phaseblockData> phasedata_ptr(new phaseblockData(clusterdata_ptr));

    // superclusters, contigs in superclusterData's order (out_ctgs: indices into the case's contigs)
    std::map<std::string, int> ctg_index;
    for (size_t k = 0; k < c.ctg_names.size(); k++) ctg_index[c.ctg_names[k]] = int(k);
    for (const char *f : {"out_ctgs", "sc_off", "sc_beg", "sc_end", "sc_phase", "sc_orig_dist", "sc_swap_dist", "sc_phase_set", "pb_phase",
                          "brk_off", "brk0", "brk1", "brk2", "brk3", "pb_off", "phase_blocks", "sw_off", "switches", "fl_off", "flips"}) out.touch(f);
    for (const char *f : {"sc_off", "brk_off", "pb_off", "sw_off", "fl_off"}) out.put1(f, 0);
    int64_t n_sc = 0, n_brk = 0, n_pb = 0, n_sw = 0, n_fl = 0;
    for (const std::string &name : clusterdata_ptr->contigs) {
        out.put1("out_ctgs", ctg_index.at(name));
        const ctgSuperclusters &s = *clusterdata_ptr->superclusters.at(name);
        // the reference keeps a sentinel entry behind a contig's last supercluster: the first n entries are the superclusters
        auto first_n = [&](const std::vector<int> &v) { return std::vector<int>(v.begin(), v.begin() + std::min<size_t>(v.size(), size_t(s.n))); };
        out.put("sc_beg", first_n(s.begs)); out.put("sc_end", first_n(s.ends)); out.put("sc_phase", first_n(s.sc_phase));
        out.put("sc_orig_dist", first_n(s.orig_phase_dist)); out.put("sc_swap_dist", first_n(s.swap_phase_dist));
        out.put("sc_phase_set", first_n(s.phase_sets)); out.put("pb_phase", first_n(s.pb_phase));
        if (int(s.phase_sets.size()) < s.n) { fprintf(stderr, "ref_harness: phase sets shorter than the superclusters\n"); exit(2); }
        for (int slot = 0; slot < 4; slot++) out.put("brk" + std::to_string(slot), s.superclusters[slot >> 1][slot & 1]);
        n_sc += s.n; n_brk += int64_t(s.superclusters[0][0].size());
        const ctgPhaseblocks &pb = *phasedata_ptr->phase_blocks.at(name);
        out.put("phase_blocks", pb.phase_blocks); out.put("switches", pb.switches); out.put("flips", pb.flips);
        n_pb += int64_t(pb.phase_blocks.size()); n_sw += int64_t(pb.switches.size()); n_fl += int64_t(pb.flips.size());
        out.put1("sc_off", n_sc); out.put1("brk_off", n_brk); out.put1("pb_off", n_pb); out.put1("sw_off", n_sw); out.put1("fl_off", n_fl);
    }

    // the six per-variant columns, per hap slot and phasing, contigs in the case's order
    for (int slot = 0; slot < 4; slot++)
        for (int w = 0; w < PHASES; w++) {
            const std::string p = "p" + std::to_string(slot) + "_" + std::to_string(w) + "_";
            for (const char *f : {"errtype", "sync_group", "callq", "ref_ed", "query_ed", "credit"}) out.touch(p + f);
            for (const std::string &name : c.ctg_names) {
                auto &m = c.callset[slot >> 1]->variants[slot & 1];
                auto it = m.find(name);
                if (it == m.end()) continue;
                const ctgVariants &v = *it->second;
                out.put(p + "errtype", v.errtypes[w]); out.put(p + "sync_group", v.sync_group[w]); out.put_bits(p + "callq", v.callq[w]);
                out.put(p + "ref_ed", v.ref_ed[w]); out.put(p + "query_ed", v.query_ed[w]); out.put_bits(p + "credit", v.credit[w]);
            }
        }
    if (g.realign_query || g.realign_truth) put_variant_columns(c, 4, out);

    // what edits.tsv is written from
    if (g.distance) {
        for (const char *f : {"ed_ctg", "ed_pos", "ed_hap", "ed_type", "ed_len", "ed_sc", "ed_min_qual", "ed_max_qual"}) out.touch(f);
        for (int k = 0; k < edits.n; k++) out.put1("ed_ctg", ctg_index.at(edits.ctgs[k]));
        out.put("ed_pos", edits.poss); out.put("ed_hap", edits.haps); out.put("ed_type", edits.types); out.put("ed_len", edits.lens);
        out.put("ed_sc", edits.superclusters); out.put("ed_min_qual", edits.min_quals); out.put("ed_max_qual", edits.max_quals);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: ref_harness swg|ed|cluster|chain|realign <case file> <result file>\n");
        return 2;
    }
    const std::string cmd = argv[1];
    Records in, out;
    in.read(argv[2]);
    int rc;
    if (cmd == "swg") rc = run_swg(in, out);
    else if (cmd == "ed") rc = run_ed(in, out);
    else if (cmd == "cluster") rc = run_cluster(in, out, argv[2]);
    else if (cmd == "chain") rc = run_chain(in, out, argv[2]);
    else if (cmd == "realign") rc = run_realign(in, out, argv[2]);
    else { fprintf(stderr, "ref_harness: unknown subcommand '%s'\n", cmd.data()); return 2; }
    if (rc == 0) out.write(argv[3]);
    return rc;
}
