// distance_model.cpp -- CPU model of the alignment-distance metrics (include/vcfdist_distance.h), written for the tests:
// the affine-gap wavefront recurrence with every row kept (no band, no ring), the backtrack over its pointer flags,
// count_dist, the edit-record rules and the three output files, restated plainly so that the GPU path and the report
// writers can be checked against something that shares none of their code.  Compiled with g++ into a temporary
// directory by tests/test_distance_model.py and loaded with ctypes.
//
// Rules restated (vcfdist v2.6.4 semantics):
//   - three matrices SUB / INS / DEL of offsets along the query, -2 = unset; score 0 holds -1 on the main diagonal;
//   - a cell takes a candidate when candidate >= current and ORs the candidate's pointer flag (INS 1, DEL 2, MAT 4, SUB 8),
//     so one cell can carry several flags;
//   - per score: INS then DEL close into SUB, then SUB extends along matches, stopping at the first diagonal that ends;
//   - the backtrack prefers, in SUB: INS, DEL, SUB, MAT; in INS / DEL: extend, then open;
//   - distance counts SUB, INS and DEL steps; records: a run is written when the next one starts, a SUB run one record
//     per base, so the run open at the end is counted but never written.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>

namespace {

const int NONE = -2;
enum { S = 0, I = 1, D = 2 };
enum { F_INS = 1, F_DEL = 2, F_MAT = 4, F_SUB = 8 };

struct Rec { int sc, hap, pos, type, len, minq, maxq; };

struct Grid {
    int nd;
    std::vector<std::vector<int>> off[3];
    std::vector<std::vector<uint8_t>> flag[3];
    void add_row() {
        for (int m = 0; m < 3; m++) { off[m].emplace_back(nd, NONE); flag[m].emplace_back(nd, 0); }
    }
    int get(int m, int s, int d) const { return s < 0 ? NONE : off[m][s][d]; }
};

// score and full history of aligning a (query) against b (truth); false if it does not end within a generous bound
bool forward(const std::string &a, const std::string &b, int x, int o, int e, Grid &G, int &score) {
    const int na = int(a.size()), nb = int(b.size());
    G.nd = na + nb - 1;
    G.add_row();
    G.off[S][0][na - 1] = -1;
    G.flag[S][0][na - 1] = F_MAT;
    const long bound = long(x + o + e) * (na + nb) + 1;
    for (int s = 0;; s++) {
        for (int m : {I, D})
            for (int d = 0; d < G.nd; d++) {
                const int v = G.off[m][s][d], k = d + 1 - na;
                if (v >= 0 && v < na && k + v >= 0 && k + v < nb && v >= G.off[S][s][d]) {
                    G.off[S][s][d] = v;
                    G.flag[S][s][d] |= (m == I ? F_INS : F_DEL);
                }
            }
        for (int d = 0; d < G.nd; d++) {
            int v = G.off[S][s][d];
            const int k = d + 1 - na;
            while (v != NONE && k + v >= -1 && v < na - 1 && k + v < nb - 1 && a[v + 1] == b[k + v + 1]) v++;
            G.off[S][s][d] = v;
            if (v == na - 1 && v + k == nb - 1) { score = s; return true; }
        }
        if (s + 1 > bound) return false;
        G.add_row();
        const int t = s + 1;
        for (int d = 0; d < G.nd; d++) {
            const int k = d + 1 - na;
            auto take = [&](int m, int cand, int f) {
                if (cand >= G.off[m][t][d]) { G.off[m][t][d] = cand; G.flag[m][t][d] |= f; }
            };
            int p;
            if (t >= x && (p = G.get(S, t - x, d)) != NONE && p + 1 < na && k + p + 1 < nb) take(S, p + 1, F_SUB);
            if (t >= o + e && d > 0 && (p = G.get(S, t - o - e, d - 1)) != NONE && k + p < nb) take(D, p, F_SUB);
            if (t >= o + e && d < G.nd - 1 && (p = G.get(S, t - o - e, d + 1)) != NONE && p + 1 < na && k + p + 1 < nb && k + p + 1 >= 0)
                take(I, p + 1, F_SUB);
            if (t >= e && d > 0 && (p = G.get(D, t - e, d - 1)) != NONE && k + p < nb) take(D, p, F_DEL);
            if (t >= e && d < G.nd - 1 && (p = G.get(I, t - e, d + 1)) != NONE && p + 1 < na && k + p + 1 < nb && k + p + 1 >= 0)
                take(I, p + 1, F_INS);
        }
    }
}

// the CIGAR steps from the end of the (reversed) strings back to their start: F_MAT / F_SUB / F_INS / F_DEL, one per step
bool backtrack(int na, int nb, const Grid &G, int s, int x, int o, int e, std::vector<int> &steps) {
    int qi = na - 1, ri = nb - 1, m = S;
    while (qi >= 0 || ri >= 0) {
        if (s < 0) return false;
        const int d = na - 1 + ri - qi;
        const uint8_t f = G.flag[m][s][d];
        auto diag_to = [&](int stop) {        // walk the diagonal down to query offset `stop`
            while (qi > stop) {
                steps.push_back(F_MAT); qi--; ri--;
                if (qi < 0 || ri < 0) return false;
            }
            return true;
        };
        if (m == S) {
            if (f & F_INS) { if (!diag_to(G.off[I][s][d])) return false; m = I; }
            else if (f & F_DEL) { if (!diag_to(G.off[D][s][d])) return false; m = D; }
            else if (f & F_SUB) {
                if (s - x < 0) return false;
                if (!diag_to(G.off[S][s - x][d] + 1)) return false;
                steps.push_back(F_SUB); qi--; ri--; s -= x;
            } else if (f & F_MAT) {
                while (qi >= 0 && ri >= 0) { steps.push_back(F_MAT); qi--; ri--; }
                if (qi >= 0 || ri >= 0) return false;
            } else return false;
        } else {
            const int own = m == I ? F_INS : F_DEL;
            if (!(f & (own | F_SUB))) return false;
            steps.push_back(own);
            if (m == I) qi--; else ri--;
            if (f & own) s -= e; else { s -= o + e; m = S; }
        }
        if (!(qi == -1 && ri == -1) && (qi < 0 || ri < 0)) return false;
    }
    return true;
}

// one alignment job -> distance and records
bool job(std::string a, std::string b, int x, int o, int e, int beg, int sc, int hap, int minq, int maxq, int &dist, std::vector<Rec> &out) {
    if (a.empty() || b.empty()) return false;
    std::reverse(a.begin(), a.end());
    std::reverse(b.begin(), b.end());
    Grid G;
    int s = 0;
    if (!forward(a, b, x, o, e, G, s)) return false;
    std::vector<int> steps;
    if (!backtrack(int(a.size()), int(b.size()), G, s, x, o, e, steps)) return false;
    // steps are already in forward order (the strings were reversed)
    dist = 0;
    for (int st : steps) dist += st != F_MAT;
    int pos = beg, run = F_MAT, len = 0;
    for (int st : steps) {
        if (st != run) {
            if (run == F_SUB) out.push_back({sc, hap, pos - 1, 1, 1, minq, maxq});
            if (run == F_INS) out.push_back({sc, hap, pos, 2, len, minq, maxq});
            if (run == F_DEL) out.push_back({sc, hap, pos - len, 3, len, minq, maxq});
            run = st; len = 0;
        } else if (st == F_SUB) {
            out.push_back({sc, hap, pos - 1, 1, 1, minq, maxq});
        }
        len++;
        if (st != F_INS) pos++;
    }
    return true;
}

struct Slot {
    const int64_t *off; const int32_t *pos; const uint8_t *type; const float *qual;
    const int32_t *ref_len, *alt_len; const int64_t *alt_off; const uint8_t *pool;
};

// the haplotype string of a region with the variants of quality >= minq applied
std::string hap_string(const uint8_t *ctg, int64_t ctg_len, int beg, int end, const Slot &h, int sc, float minq, bool &ok) {
    std::string out;
    end = int(std::min<int64_t>(end, ctg_len - 1));
    int64_t v = h.off[sc];
    for (int p = beg; p <= end;) {
        if (v < h.off[sc + 1] && h.pos[v] == p) {
            if (h.qual[v] >= minq) {
                const char *alt = reinterpret_cast<const char *>(h.pool + h.alt_off[v]);
                if (h.type[v] == 2) out.append(alt, size_t(h.alt_len[v]));
                else if (h.type[v] == 3) p += h.ref_len[v];
                else { out.push_back(alt[0]); p++; }
            }
            v++;
        } else {
            const int stop = v < h.off[sc + 1] ? h.pos[v] : end + 1;
            if (stop < p) { ok = false; return out; }
            out.append(reinterpret_cast<const char *>(ctg) + p, size_t(stop - p));
            p = stop;
        }
    }
    return out;
}

std::vector<Rec> g_recs;
std::vector<int> g_jobs;    // 5 ints per job: sc, hap, minq, maxq, dist

float qscore(double p) { return float(std::min(100.0, std::max(0.0, -10 * std::log10(p)))); }

}  // namespace

extern "C" {

// one job on explicit strings (forward orientation): returns the number of records (written to rec[7 * k], up to cap),
// -1 when the alignment fails
int dm_job(const char *q, const char *t, int x, int o, int e, int beg, int sc, int hap, int minq, int maxq, int *dist, int *rec, int cap) {
    std::vector<Rec> out;
    if (!job(q, t, x, o, e, beg, sc, hap, minq, maxq, *dist, out)) return -1;
    for (int k = 0; k < int(out.size()) && k < cap; k++) {
        const Rec &r = out[size_t(k)];
        const int v[7] = {r.sc, r.hap, r.pos, r.type, r.len, r.minq, r.maxq};
        std::memcpy(rec + 7 * k, v, sizeof(v));
    }
    return int(out.size());
}

// a whole batch (contigs concatenated as in vpr_variants): slot columns in cols[slot * 8 + {off, pos, type, qual, ref_len, alt_len, alt_off, pool}];
// skip[sc] != 0 drops a supercluster.  Returns the number of jobs (read with dm_jobs / dm_records), -1 on a failed job.
long dm_run(const uint8_t *ctg_seq, const int64_t *ctg_off, const int32_t *sc_ctg, int n_sc, const int32_t *sc_beg, const int32_t *sc_end,
            void **cols, const int32_t *sc_phase, const uint8_t *skip, int x, int o, int e, int max_qual) {
    g_recs.clear(); g_jobs.clear();
    Slot sl[4];
    for (int k = 0; k < 4; k++) {
        void **c = cols + 8 * k;
        sl[k] = Slot{static_cast<const int64_t *>(c[0]), static_cast<const int32_t *>(c[1]), static_cast<const uint8_t *>(c[2]),
                     static_cast<const float *>(c[3]), static_cast<const int32_t *>(c[4]), static_cast<const int32_t *>(c[5]),
                     static_cast<const int64_t *>(c[6]), static_cast<const uint8_t *>(c[7])};
    }
    for (int sc = 0; sc < n_sc; sc++) {
        if (skip[sc]) continue;
        const uint8_t *ctg = ctg_seq + ctg_off[sc_ctg[sc]];
        const int64_t ctg_len = ctg_off[sc_ctg[sc] + 1] - ctg_off[sc_ctg[sc]];
        for (int hap = 0; hap < 2; hap++) {
            const int ts = 2 + (sc_phase[sc] == 1 ? 1 - hap : hap);
            bool ok = true;
            const std::string truth = hap_string(ctg, ctg_len, sc_beg[sc], sc_end[sc], sl[ts], sc, 0.0f, ok);
            std::set<int> th;
            for (int64_t v = sl[hap].off[sc]; v < sl[hap].off[sc + 1]; v++) th.insert(int(sl[hap].qual[v] + 1.0f));
            th.insert(max_qual + 2);
            int prev = 0;
            for (int qual : th) {
                const std::string query = hap_string(ctg, ctg_len, sc_beg[sc], sc_end[sc], sl[hap], sc, float(prev), ok);
                int dist = 0;
                if (!ok || !job(query, truth, x, o, e, sc_beg[sc], sc, hap, prev, qual, dist, g_recs)) return -1;
                g_jobs.insert(g_jobs.end(), {sc, hap, prev, qual, dist});
                prev = qual;
            }
        }
    }
    return long(g_jobs.size() / 5);
}
void dm_jobs(int *out) { std::copy(g_jobs.begin(), g_jobs.end(), out); }
long dm_n_records() { return long(g_recs.size()); }
void dm_records(int *out) {
    for (size_t k = 0; k < g_recs.size(); k++) {
        const Rec &r = g_recs[k];
        const int v[7] = {r.sc, r.hap, r.pos, r.type, r.len, r.minq, r.maxq};
        std::memcpy(out + 7 * k, v, sizeof(v));
    }
}

// the three files and the summary, counting every record at every quality (the plain quadratic way).  rec: 7 ints per record
// as above; ctg_of[k]: contig name of record k.  Files under prefix when write != 0; the summary text into summary.
int dm_write(const char *prefix, const char *const *ctg_of, const int *rec, long n, int min_qual, int max_qual, int x, int o, int e,
             int verbosity, int write, char *summary, long cap) {
    static const char *T1[] = {"REF", "SNP", "INS", "DEL", "CPX"};
    static const char *T2[] = {"ALL", "SNP", "INS", "DEL", "INDEL"};
    auto in_type = [](int type, int cat) { return cat == 0 || type == cat || (cat == 4 && (type == 2 || type == 3)); };
    auto live = [&](long k, int q) { return q >= rec[7 * k + 5] && q < rec[7 * k + 6]; };
    auto ed = [&](int q, int cat) { int v = 0; for (long k = 0; k < n; k++) if (live(k, q) && in_type(rec[7 * k + 3], cat)) v += rec[7 * k + 4]; return v; };
    auto de = [&](int q, int cat) { int v = 0; for (long k = 0; k < n; k++) if (live(k, q) && in_type(rec[7 * k + 3], cat)) v++; return v; };
    auto sc = [&](int q) {
        int v = 0;
        for (long k = 0; k < n; k++) if (live(k, q)) v += rec[7 * k + 3] == 1 ? x : o + e * rec[7 * k + 4];
        return v;
    };
    std::string pre = prefix ? prefix : "";
    FILE *f = write ? fopen((pre + "distance.tsv").c_str(), "w") : nullptr;
    if (write && !f) return -1;
    if (f) fprintf(f, "MIN_QUAL\tSUB_DE\tINS_DE\tDEL_DE\tSUB_ED\tINS_ED\tDEL_ED\tDISTINCT_EDITS\tEDIT_DIST\tALN_SCORE\tALN_QSCORE\n");
    const int top = max_qual + 1;
    const int orig = sc(top);
    int orig_ed[5], orig_de[5], best_q[5];
    double best[5];
    for (int c = 0; c < 5; c++) { orig_ed[c] = ed(top, c); orig_de[c] = de(top, c); best[c] = std::numeric_limits<double>::max(); best_q[c] = 0; }
    for (int q = min_qual; q <= top; q++) {
        int E[5], N[5];
        for (int c = 0; c < 5; c++) {
            E[c] = ed(q, c); N[c] = de(q, c);
            const double v = double(E[c]) * N[c];
            if (v < best[c]) { best[c] = v; best_q[c] = q; }
        }
        if (f) fprintf(f, "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%f\n", q, N[1], N[2], N[3], E[1], E[2], E[3], N[0], E[0], sc(q),
                       qscore(double(sc(q)) / orig));
    }
    if (f) fclose(f);
    FILE *g = write ? fopen((pre + "distance-summary.tsv").c_str(), "w") : nullptr;
    if (write && !g) return -1;
    if (g) fprintf(g, "VAR_TYPE\tTHRESHOLD\tMIN_QUAL\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE\n");
    std::string txt = "ALIGNMENT DISTANCE SUMMARY\n";
    char line[512];
    for (int c = 0; c < 5; c++) {
        if ((verbosity == 0 && c != 0) || (verbosity == 1 && (c == 2 || c == 3))) continue;     // summary file and text alike
        txt += c == 0 ? "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\tALN_QSCORE\n"
                      : "\nTYPE\tTHRESHOLD\tEDIT_DIST\tDISTINCT_EDITS\tED_QSCORE\tDE_QSCORE\n";
        const int qs[3] = {min_qual, best_q[c], top};
        const char *names[3] = {"NONE", "BEST", "REF "};
        for (int i = 0; i < 3; i++) {
            const int q = qs[i];
            const float eq = qscore(double(ed(q, c)) / orig_ed[c]), dq = qscore(double(de(q, c)) / orig_de[c]);
            const float aq = c == 0 ? qscore(double(sc(q)) / orig) : 0;
            if (g) fprintf(g, "%s\t%s\t%d\t%d\t%d\t%f\t%f\t%f\n", T2[c], names[i], q, ed(q, c), de(q, c), eq, dq, aq);
            if (c == 0) snprintf(line, sizeof(line), "%s\t%s Q >= %d\t%-16d%-16d%f\t%f\t%f\n", T2[c], names[i], q, ed(q, c), de(q, c), eq, dq, aq);
            else snprintf(line, sizeof(line), "%s\t%s Q >= %d\t%-16d%-16d%f\t%f\n", T2[c], names[i], q, ed(q, c), de(q, c), eq, dq);
            txt += line;
        }
    }
    if (g) fclose(g);
    if (write) {
        FILE *h = fopen((pre + "edits.tsv").c_str(), "w");
        if (!h) return -1;
        fprintf(h, "CONTIG\tSTART\tHAP\tTYPE\tSIZE\tSUPERCLUSTER\tMIN_QUAL\tMAX_QUAL\n");
        for (long k = 0; k < n; k++)
            fprintf(h, "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n", ctg_of[k], rec[7 * k + 2], rec[7 * k + 1], T1[rec[7 * k + 3]], rec[7 * k + 4],
                    rec[7 * k], rec[7 * k + 5], rec[7 * k + 6]);
        fclose(h);
    }
    if (summary && cap > 0) snprintf(summary, size_t(cap), "%s", txt.c_str());
    return int(txt.size());
}

}  // extern "C"

extern "C" {
// the CIGAR steps of one job in forward order (F_MAT 4, F_SUB 8, F_INS 1, F_DEL 2); -1 when the alignment fails
int dm_steps(const char *q, const char *t, int x, int o, int e, int *out, int cap) {
    std::string a(q), b(t);
    if (a.empty() || b.empty()) return -1;
    std::reverse(a.begin(), a.end());
    std::reverse(b.begin(), b.end());
    Grid G;
    int s = 0;
    std::vector<int> steps;
    if (!forward(a, b, x, o, e, G, s) || !backtrack(int(a.size()), int(b.size()), G, s, x, o, e, steps)) return -1;
    for (int k = 0; k < int(steps.size()) && k < cap; k++) out[k] = steps[size_t(k)];
    return int(steps.size());
}
}
