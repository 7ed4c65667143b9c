// pr_realign.hip -- the realignment of one (contig, hap) (include/vcfdist_realign.h): wf_swg_realign (dist.cpp:2496-2594) on the
// device, left_shift (variant.cpp:57-127) on the host.
//
// A job is one cluster.  Steps, on one stream of the chosen device:
//   k_rl_jobs      one thread per cluster: the region [poss[first] - 1, poss[last] + rlens[last] + 1), its checks (EDGE, an
//                  inconsistent generate_str -> ERROR), the string lengths and the pass-1 scratch size
//   k_rl_wave<false / true>  pass 1 / pass 2, one wavefront per job: the reversed haplotype (generate_str) and reversed reference
//                  (substr, clamped at the contig's end) and the recurrence of pr_swg.h, for the score and then with history
//   k_rl_back      one thread per job: the walk of pr_swg.h with add_variants as a state machine over its forward steps (one SUB
//                  record per base, then DEL runs and INS runs).  Launched twice: count (records, allele bytes), then, after a
//                  scan of both, write the records and copy their allele bytes out of the arena in the same round
// The rounds are pr_swg.h's.  The host then merges the records with the kept clusters' variants and runs left_shift.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pr_plan.h"
#include "pr_swg.h"
#include "../../include/vcfdist_pr.h"
#include "../../include/vcfdist_realign.h"

namespace {

using namespace swg;

struct RTab {
    const uint8_t *seq;
    int32_t ctg_len, n_cl;
    const int32_t *pos, *rlen, *ref_len, *alt_len;
    const uint8_t *type;
    const int64_t *alt_off;
    const uint8_t *pool;
    const int32_t *var_beg;
};

struct RJob { int32_t beg, end, q_len, t_len; };                   // end: the reference's (unclamped) region end
struct RRec { int32_t pos, rlen, ref_len, alt_len; int64_t boff; uint8_t type, pad[7]; };

// generate_str (dist.cpp:81-138) of cluster c over [beg, end): emit(src, n) for every piece in order.  false where the reference
// ERRORs or throws: the walk goes backwards (overlapping variants) or a reference piece starts past the contig's end
template <typename F>
__device__ bool rl_walk(const RTab &T, int c, int beg, int end, F emit) {
    int v = T.var_beg[c];
    const int ve = T.var_beg[c + 1];
    for (int pos = beg; pos < end;) {
        if (v < ve && pos == T.pos[v]) {
            const int type = T.type[v];
            if (type == VPR_TYPE_INS) emit(T.pool + T.alt_off[v], T.alt_len[v]);
            else if (type == VPR_TYPE_DEL) pos += T.ref_len[v];
            else { emit(T.pool + T.alt_off[v], T.alt_len[v]); pos++; }
            v++;
        } else {
            const int stop = v < ve ? min(end, T.pos[v]) : end;
            if (stop < pos || pos > T.ctg_len) return false;
            emit(T.seq + pos, min(stop, T.ctg_len) - pos);        // (substr clamps at the end)
            pos = stop;
        }
    }
    return true;
}

__global__ void k_rl_jobs(RTab T, RJob *jobs, int64_t *need, uint8_t *status, int P) {
    const int c = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= T.n_cl) return;
    const int b = T.var_beg[c], e = T.var_beg[c + 1];
    RJob J{0, 0, 0, 0};
    uint8_t st = 0;
    if (e <= b) {
        st = VRL_ST_ERROR;
    } else {
        J.beg = T.pos[b] - 1;
        J.end = T.pos[e - 1] + T.rlen[e - 1] + 1;
        if (J.beg < 0) {
            st = VRL_ST_EDGE;
        } else if (J.beg > T.ctg_len) {
            st = VRL_ST_ERROR;
        } else {
            int n = 0;
            const bool ok = rl_walk(T, c, J.beg, J.end, [&](const uint8_t *, int k) { n += k; });
            J.q_len = n;
            J.t_len = min(J.end, T.ctg_len) - J.beg;
            if (!ok || J.q_len <= 0 || J.t_len <= 0) st = VRL_ST_ERROR;
        }
    }
    jobs[c] = J;
    status[c] = st;
    need[c] = st ? 0 : need1(J.q_len, J.t_len, P);
}

template <bool HIST>
__global__ void __launch_bounds__(64) k_rl_wave(RTab T, const RJob *__restrict__ jobs, int64_t j0, int64_t n,
                                                 const int64_t *__restrict__ slice, uint8_t *arena, uint8_t *status, int32_t *score,
                                                 int64_t *need2_out, int64_t *cells_out, DPen pen) {
    const int64_t j = j0 + int64_t(blockIdx.x);
    if (int64_t(blockIdx.x) >= n) return;
    if (status[j]) return;
    const RJob J = jobs[j];
    auto load = [&](uint8_t *qs, uint8_t *ts, int lane) {      // both strings reversed (dist.cpp:2560-2561)
        int m = 0;
        rl_walk(T, int(j), J.beg, J.end, [&](const uint8_t *src, int k) {
            for (int c = lane; c < k; c += 64) qs[J.q_len - 1 - (m + c)] = src[c];
            m += k;
        });
        const uint8_t *r = T.seq + J.beg;
        for (int c = lane; c < J.t_len; c += 64) ts[J.t_len - 1 - c] = r[c];
    };
    const WaveOut W = swg_wave<HIST>(J.q_len, J.t_len, pen, arena + slice[j], HIST ? score[j] : 0, HIST ? cells_out[j] : 0, load);
    if (threadIdx.x != 0) return;
    if (W.failed) { status[j] |= VRL_ST_ERROR; return; }
    if (!HIST) {
        score[j] = W.s;
        cells_out[j] = W.cells;
        need2_out[j] = need2(J.q_len, J.t_len, W.s, W.cells);
    }
}

// add_variants (variant.cpp:332-391) over the walk of one job per thread.  WRITE = false: records and allele bytes per job;
// WRITE = true: the records and their bytes (REF then ALT) at the offsets the scans gave.
template <bool WRITE>
__global__ void k_rl_back(const RJob *__restrict__ jobs, int64_t j0, int64_t n, const int64_t *__restrict__ slice, const uint8_t *arena,
                          uint8_t *status, const int32_t *score, const int64_t *cells_in, int64_t *n_rec, int64_t *n_byte,
                          const int64_t *rec_off, const int64_t *byte_off, int64_t rec_base, int64_t byte_base, RRec *rec_out,
                          uint8_t *pool_out, DPen pen) {
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t j = j0 + k;
    if (status[j]) { if (!WRITE) { n_rec[k] = 0; n_byte[k] = 0; } return; }
    const RJob J = jobs[j];
    const int q = J.q_len, t = J.t_len;
    const uint8_t *base = arena + slice[j];
    const uint8_t *qs = base, *ts = base + pad16(q);
    int64_t nr = 0, nb = 0;
    const int64_t ro = WRITE ? rec_off[k] + rec_base : 0, bo = WRITE ? byte_off[k] + byte_base : 0;
    // one record: ref bytes ts[rr], ts[rr - 1] ... (forward order), then alt bytes qs[qq], qs[qq - 1] ...
    auto rec = [&](int type, int pos, int rlen, int ref_len, int rr, int alt_len, int qq) {
        if (WRITE) {
            RRec R;
            R.pos = pos; R.rlen = rlen; R.ref_len = ref_len; R.alt_len = alt_len; R.boff = bo + nb; R.type = uint8_t(type);
            for (int p = 0; p < 7; p++) R.pad[p] = 0;
            rec_out[ro + nr] = R;
            uint8_t *dst = pool_out + bo + nb;
            for (int c = 0; c < ref_len; c++) dst[c] = ts[rr - c];
            for (int c = 0; c < alt_len; c++) dst[ref_len + c] = qs[qq - c];
        }
        nr++;
        nb += ref_len + alt_len;
    };
    int run = 0, run_len = 0, run_q = 0, run_r = 0;          // the open INS / DEL run: its first step's (reversed) indices
    auto flush = [&]() {
        if (run == DP_DEL) rec(VPR_TYPE_DEL, J.beg + (t - 1 - run_r), run_len, run_len, run_r, 0, 0);
        else if (run == DP_INS) rec(VPR_TYPE_INS, J.beg + (t - 1 - run_r), 0, 0, 0, run_len, run_q);
        run = 0;
    };
    const bool ok = swg_walk(base, q, t, score[j], cells_in[j], pen, [&](int type, int qi, int ri) {
        if (type != run) flush();
        if (type == DP_SUB) rec(VPR_TYPE_SUB, J.beg + (t - 1 - ri), 1, 1, ri, 1, qi);
        else if (type == DP_INS || type == DP_DEL) {
            if (run != type) { run = type; run_len = 0; run_q = qi; run_r = ri; }
            run_len++;
        }
    });
    flush();
    if (WRITE) return;
    if (!ok) { status[j] |= VRL_ST_ERROR; n_rec[k] = 0; n_byte[k] = 0; return; }
    n_rec[k] = nr;
    n_byte[k] = nb;
}

double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the call's device buffers, events and stream, released on every return path
struct Dev {
    std::vector<void *> allocs;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~Dev() {
        if (st) (void)hipStreamSynchronize(st);
        for (void *p : allocs) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
    template <typename T>
    T *alloc(size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        allocs.push_back(p);
        return static_cast<T *>(p);
    }
    void release(void *p) {
        if (!p) return;
        auto it = std::find(allocs.begin(), allocs.end(), p);
        if (it != allocs.end()) { (void)hipFree(p); allocs.erase(it); }
    }
    template <typename T>
    T *copy(const T *src, size_t n) {
        T *p = alloc<T>(n);
        if (p && n && hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
        return p;
    }
    double ms() {
        float m = 0;
        (void)hipEventSynchronize(ev[1]);
        (void)hipEventElapsedTime(&m, ev[0], ev[1]);
        return m;
    }
};

// left_shift (variant.cpp:57-127) over one (contig, hap)'s columns; alleles are rotated in place in the pool
void left_shift(vrl_result *r, const uint8_t *seq, int32_t ctg_len) {
    for (int i = 0; i < r->n; i++) {
        const int t = r->type[i];
        if (t != VPR_TYPE_INS && t != VPR_TYPE_DEL) continue;
        uint8_t *a = r->pool + (t == VPR_TYPE_INS ? r->alt_off[i] : r->ref_off[i]);
        const int len = t == VPR_TYPE_INS ? r->alt_len[i] : r->ref_len[i];
        if (len <= 0) continue;
        while (r->pos[i] > 0 && r->pos[i] - 1 < ctg_len && (i == 0 || r->pos[i] > r->pos[i - 1] + r->rlen[i - 1] + 1)) {
            const uint8_t base = seq[r->pos[i] - 1];
            if (base != a[len - 1]) break;
            memmove(a + 1, a, size_t(len - 1));
            a[0] = base;
            r->pos[i]--;
        }
    }
    for (int i = 0; i + 1 < r->n; i++) {
        if (r->ref_len[i] && r->pos[i + 1] == r->pos[i]) {           // every column but pos and phase_set
            std::swap(r->rlen[i], r->rlen[i + 1]);
            std::swap(r->type[i], r->type[i + 1]);
            std::swap(r->ref_len[i], r->ref_len[i + 1]);
            std::swap(r->ref_off[i], r->ref_off[i + 1]);
            std::swap(r->alt_len[i], r->alt_len[i + 1]);
            std::swap(r->alt_off[i], r->alt_off[i + 1]);
            std::swap(r->orig_gt[i], r->orig_gt[i + 1]);
            std::swap(r->gt_qual[i], r->gt_qual[i + 1]);
            std::swap(r->var_qual[i], r->var_qual[i + 1]);
        }
    }
}

template <typename T>
T *host_alloc(size_t n) { return static_cast<T *>(calloc(std::max<size_t>(n, 1), sizeof(T))); }

}  // namespace

extern "C" void vrl_result_free(vrl_result *r) {
    if (!r) return;
    void *ps[] = {r->pos, r->rlen, r->type, r->ref_len, r->alt_len, r->ref_off, r->alt_off, r->pool, r->var_qual, r->gt_qual,
                  r->phase_set, r->orig_gt, r->cluster_status};
    for (void *p : ps) free(p);
    free(r);
}

extern "C" int vrl_realign(const vcl_hap_seq *hs, const float *var_qual, const float *gt_qual, const int32_t *phase_set,
                           const uint8_t *orig_gt, const vcl_clusters *cl, const uint8_t *ctg_seq, int32_t ctg_len, const vrl_config *cfg,
                           int32_t device, vrl_result **out) {
    if (!hs || !var_qual || !phase_set || !cl || !cfg || !out || ctg_len < 0 || (ctg_len > 0 && !ctg_seq)) return VRL_ERR_ARG;
    if (cfg->sub < 1 || cfg->open < 0 || cfg->extend < 1 || cfg->max_qual < 0) return VRL_ERR_ARG;
    *out = nullptr;
    const double t_wall = wall_ms();
    const vcl_hap &h = hs->cols;
    const int n_var = h.n_var;
    const int n_cl = n_var > 0 ? cl->n : 0;
    if (n_var < 0 || n_cl < 0 || (n_var && (!h.pos || !h.rlen || !h.type || !h.ref_len || !h.alt_len || !hs->ref_off || !hs->alt_off ||
                                            !hs->pool || !cl->var_beg)))
        return VRL_ERR_ARG;
    for (int v = 0; v < n_var; v++)
        if ((v && h.pos[v] < h.pos[v - 1]) || h.type[v] < VPR_TYPE_SUB || h.type[v] > VPR_TYPE_DEL) return VRL_ERR_ARG;
    if (n_var) {
        if (cl->var_beg[0] != 0 || cl->var_beg[n_cl] != n_var) return VRL_ERR_ARG;
        for (int c = 0; c < n_cl; c++) if (cl->var_beg[c + 1] <= cl->var_beg[c]) return VRL_ERR_ARG;
    }
    vrl_info I;
    memset(&I, 0, sizeof(I));
    I.n_clusters = n_cl;
    const DPen pen{cfg->sub, cfg->open, cfg->extend};
    const int P = std::max(pen.x, pen.o + pen.e) + 1;

    std::vector<uint8_t> st(static_cast<size_t>(n_cl), 0);
    std::vector<int64_t> nrec(static_cast<size_t>(n_cl), 0), nbyte(static_cast<size_t>(n_cl), 0);
    std::vector<RRec> recs;
    std::vector<uint8_t> rpool;
    if (n_cl > 0) {
        Dev D;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return VRL_ERR_DEVICE;
        if (hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&D.ev[0]) != hipSuccess ||
            hipEventCreate(&D.ev[1]) != hipSuccess)
            return VRL_ERR_DEVICE;
        const double t_up = wall_ms();
        int64_t pool_len = 1;
        for (int v = 0; v < n_var; v++) pool_len = std::max<int64_t>(pool_len, hs->alt_off[v] + h.alt_len[v]);
        RTab T;
        T.ctg_len = ctg_len; T.n_cl = n_cl;
        T.seq = D.copy(ctg_seq, size_t(ctg_len));
        T.pos = D.copy(h.pos, size_t(n_var)); T.rlen = D.copy(h.rlen, size_t(n_var));
        T.ref_len = D.copy(h.ref_len, size_t(n_var)); T.alt_len = D.copy(h.alt_len, size_t(n_var));
        T.type = D.copy(h.type, size_t(n_var)); T.alt_off = D.copy(hs->alt_off, size_t(n_var));
        T.pool = D.copy(hs->pool, size_t(pool_len));
        T.var_beg = D.copy(cl->var_beg, size_t(n_cl) + 1);
        const size_t nj = size_t(n_cl) + 1;
        RJob *d_jobs = D.alloc<RJob>(nj);
        int64_t *d_need1 = D.alloc<int64_t>(nj), *d_need2 = D.alloc<int64_t>(nj), *d_cells = D.alloc<int64_t>(nj), *d_slice = D.alloc<int64_t>(nj);
        int64_t *d_nrec = D.alloc<int64_t>(nj), *d_nbyte = D.alloc<int64_t>(nj), *d_roff = D.alloc<int64_t>(nj), *d_boff = D.alloc<int64_t>(nj);
        int32_t *d_score = D.alloc<int32_t>(nj);
        uint8_t *d_status = D.alloc<uint8_t>(nj);
        if (!T.seq || !T.pos || !T.rlen || !T.ref_len || !T.alt_len || !T.type || !T.alt_off || !T.pool || !T.var_beg || !d_jobs || !d_need1 ||
            !d_need2 || !d_cells || !d_slice || !d_nrec || !d_nbyte || !d_roff || !d_boff || !d_score || !d_status)
            return VRL_ERR_NOMEM;
        if (hipStreamSynchronize(D.st) != hipSuccess) return VRL_ERR_DEVICE;
        I.ms_upload = wall_ms() - t_up;

        // ---- the jobs
        (void)hipEventRecord(D.ev[0], D.st);
        hipLaunchKernelGGL(k_rl_jobs, dim3(unsigned((n_cl + 255) / 256)), dim3(256), 0, D.st, T, d_jobs, d_need1, d_status, P);
        (void)hipEventRecord(D.ev[1], D.st);
        if (hipGetLastError() != hipSuccess) return VRL_ERR_DEVICE;
        I.ms_jobs = D.ms();
        std::vector<int64_t> n1(static_cast<size_t>(n_cl));
        if (hipMemcpyAsync(n1.data(), d_need1, 8 * size_t(n_cl), hipMemcpyDeviceToHost, D.st) != hipSuccess ||
            hipMemcpyAsync(st.data(), d_status, size_t(n_cl), hipMemcpyDeviceToHost, D.st) != hipSuccess ||
            hipStreamSynchronize(D.st) != hipSuccess)
            return VRL_ERR_DEVICE;

        // ---- memory plan: half of what the device has free for one job (or the caller's limit)
        size_t fr = 0, tt = 0;
        if (hipMemGetInfo(&fr, &tt) != hipSuccess) return VRL_ERR_DEVICE;
        const int64_t plan = std::max<int64_t>(int64_t(fr) / 2, int64_t(1) << 20);
        const int64_t limit = cfg->job_bytes_limit > 0 ? std::min<int64_t>(cfg->job_bytes_limit, plan) : plan;
        const int64_t cap1 = std::min<int64_t>(cfg->round_bytes > 0 ? cfg->round_bytes : int64_t(4) << 30, limit);
        const int64_t cap2 = cfg->round_bytes > 0 ? std::min<int64_t>(cfg->round_bytes, limit) : limit;
        I.plan_bytes = limit;
        uint8_t *arena = nullptr;
        void *scan_tmp = nullptr;
        size_t scan_cap = 0;
        auto scan = [&](const int64_t *in, int64_t *o, size_t n) -> bool {
            size_t need = 0;
            if (vplan_exclusive_scan_i64(nullptr, &need, in, o, n, D.st)) return false;
            if (need > scan_cap) {
                D.release(scan_tmp);
                scan_tmp = D.alloc<uint8_t>(need);
                scan_cap = scan_tmp ? need : 0;
                if (!scan_tmp) return false;
            }
            return vplan_exclusive_scan_i64(scan_tmp, &need, in, o, n, D.st) == 0;
        };
        RRec *d_recs = nullptr;
        uint8_t *d_pool = nullptr;
        int64_t rec_cap = 0, pool_cap = 0, got[2] = {0, 0};
        // the backtrack of a sub-round: count records and bytes, scan both, write them into buffers of the sub-round's own
        auto back = [&](int64_t c, int64_t m, uint8_t *ar) -> int {
            const unsigned gb = unsigned((m + 63) / 64);
            hipLaunchKernelGGL(k_rl_back<false>, dim3(gb), dim3(64), 0, D.st, d_jobs, c, m, d_slice, ar, d_status, d_score, d_cells,
                               d_nrec, d_nbyte, d_roff, d_boff, int64_t(0), int64_t(0), d_recs, d_pool, pen);
            if (hipMemsetAsync(d_nrec + m, 0, 8, D.st) != hipSuccess || hipMemsetAsync(d_nbyte + m, 0, 8, D.st) != hipSuccess)
                return ROUNDS_DEVICE;
            if (!scan(d_nrec, d_roff, size_t(m) + 1) || !scan(d_nbyte, d_boff, size_t(m) + 1)) return ROUNDS_DEVICE;
            if (hipMemcpyAsync(&got[0], d_roff + m, 8, hipMemcpyDeviceToHost, D.st) != hipSuccess ||
                hipMemcpyAsync(&got[1], d_boff + m, 8, hipMemcpyDeviceToHost, D.st) != hipSuccess ||
                hipMemcpyAsync(nrec.data() + c, d_nrec, 8 * size_t(m), hipMemcpyDeviceToHost, D.st) != hipSuccess ||
                hipMemcpyAsync(nbyte.data() + c, d_nbyte, 8 * size_t(m), hipMemcpyDeviceToHost, D.st) != hipSuccess ||
                hipStreamSynchronize(D.st) != hipSuccess)
                return ROUNDS_DEVICE;
            if (got[0] > rec_cap) { D.release(d_recs); d_recs = D.alloc<RRec>(size_t(got[0])); rec_cap = d_recs ? got[0] : 0; if (!d_recs) return ROUNDS_NOMEM; }
            if (got[1] > pool_cap) { D.release(d_pool); d_pool = D.alloc<uint8_t>(size_t(got[1])); pool_cap = d_pool ? got[1] : 0; if (!d_pool) return ROUNDS_NOMEM; }
            if (got[0])
                hipLaunchKernelGGL(k_rl_back<true>, dim3(gb), dim3(64), 0, D.st, d_jobs, c, m, d_slice, ar, d_status, d_score, d_cells,
                                   d_nrec, d_nbyte, d_roff, d_boff, int64_t(0), int64_t(0), d_recs, d_pool, pen);
            return ROUNDS_OK;
        };
        // its records and bytes come down before the arena and the two buffers are reused
        auto collect = [&](int64_t, int64_t) -> int {
            const size_t r0 = recs.size(), p0 = rpool.size();
            recs.resize(r0 + size_t(got[0]));
            rpool.resize(p0 + size_t(got[1]));
            if ((got[0] && hipMemcpyAsync(recs.data() + r0, d_recs, sizeof(RRec) * size_t(got[0]), hipMemcpyDeviceToHost, D.st) != hipSuccess) ||
                (got[1] && hipMemcpyAsync(rpool.data() + p0, d_pool, size_t(got[1]), hipMemcpyDeviceToHost, D.st) != hipSuccess) ||
                hipStreamSynchronize(D.st) != hipSuccess)
                return ROUNDS_DEVICE;
            for (size_t k = r0; k < recs.size(); k++) recs[k].boff += int64_t(p0);
            return ROUNDS_OK;
        };
        Rounds R{D.st, {D.ev[0], D.ev[1]}, limit, cap1, cap2, VRL_ST_LIMIT, d_slice, d_status, d_need2};
        const int rr = R.run(
            n1, st, [&] { return hipStreamSynchronize(D.st); },
            [&](int64_t bytes) { D.release(arena); return arena = D.alloc<uint8_t>(size_t(bytes)); },
            [&](bool hist, int64_t a, int64_t n, uint8_t *ar) {
                if (hist)
                    hipLaunchKernelGGL(k_rl_wave<true>, dim3(unsigned(n)), dim3(64), 0, D.st, T, d_jobs, a, n, d_slice, ar, d_status, d_score,
                                       d_need2, d_cells, pen);
                else
                    hipLaunchKernelGGL(k_rl_wave<false>, dim3(unsigned(n)), dim3(64), 0, D.st, T, d_jobs, a, n, d_slice, ar, d_status, d_score,
                                       d_need2, d_cells, pen);
            },
            back, collect);
        if (rr) return rr == ROUNDS_NOMEM ? VRL_ERR_NOMEM : VRL_ERR_DEVICE;
        I.n_rounds = R.n_rounds; I.n_hist_rounds = R.n_hist_rounds; I.arena_bytes = R.arena_bytes;
        I.ms_score = R.ms_score; I.ms_hist = R.ms_hist; I.ms_back = R.ms_back;
    }

    // ---- merge: each cluster's records, or its original variants where it carries a status bit; then left_shift
    const double t_host = wall_ms();
    int64_t n_out = 0, pool_out = 0;
    for (int c = 0; c < n_cl; c++) {
        if (st[size_t(c)]) {
            for (int v = cl->var_beg[c]; v < cl->var_beg[c + 1]; v++) pool_out += h.ref_len[v] + h.alt_len[v];
            n_out += cl->var_beg[c + 1] - cl->var_beg[c];
        } else {
            n_out += nrec[size_t(c)];
            pool_out += nbyte[size_t(c)];
        }
    }
    if (n_out > INT32_MAX) return VRL_ERR_ARG;
    vrl_result *r = static_cast<vrl_result *>(calloc(1, sizeof(vrl_result)));
    if (!r) return VRL_ERR_NOMEM;
    r->n = int32_t(n_out);
    r->pos = host_alloc<int32_t>(size_t(n_out)); r->rlen = host_alloc<int32_t>(size_t(n_out)); r->type = host_alloc<uint8_t>(size_t(n_out));
    r->ref_len = host_alloc<int32_t>(size_t(n_out)); r->alt_len = host_alloc<int32_t>(size_t(n_out));
    r->ref_off = host_alloc<int64_t>(size_t(n_out)); r->alt_off = host_alloc<int64_t>(size_t(n_out));
    r->pool = host_alloc<uint8_t>(size_t(pool_out)); r->pool_len = pool_out;
    r->var_qual = host_alloc<float>(size_t(n_out)); r->gt_qual = host_alloc<float>(size_t(n_out));
    r->phase_set = host_alloc<int32_t>(size_t(n_out)); r->orig_gt = host_alloc<uint8_t>(size_t(n_out));
    r->n_clusters = n_cl; r->cluster_status = host_alloc<uint8_t>(size_t(n_cl));
    if (!r->pos || !r->rlen || !r->type || !r->ref_len || !r->alt_len || !r->ref_off || !r->alt_off || !r->pool || !r->var_qual ||
        !r->gt_qual || !r->phase_set || !r->orig_gt || !r->cluster_status) {
        vrl_result_free(r);
        return VRL_ERR_NOMEM;
    }
    int64_t o = 0, po = 0, rk = 0;
    for (int c = 0; c < n_cl; c++) {
        const int b = cl->var_beg[c], e = cl->var_beg[c + 1];
        r->cluster_status[c] = st[size_t(c)];
        if (st[size_t(c)]) {
            I.n_kept++;
            I.n_edge += (st[size_t(c)] & VRL_ST_EDGE) != 0; I.n_limit += (st[size_t(c)] & VRL_ST_LIMIT) != 0; I.n_error += (st[size_t(c)] & VRL_ST_ERROR) != 0;
            for (int v = b; v < e; v++, o++) {
                r->pos[o] = h.pos[v]; r->rlen[o] = h.rlen[v]; r->type[o] = h.type[v];
                r->ref_len[o] = h.ref_len[v]; r->alt_len[o] = h.alt_len[v];
                r->ref_off[o] = po; memcpy(r->pool + po, hs->pool + hs->ref_off[v], size_t(h.ref_len[v])); po += h.ref_len[v];
                r->alt_off[o] = po; memcpy(r->pool + po, hs->pool + hs->alt_off[v], size_t(h.alt_len[v])); po += h.alt_len[v];
                r->var_qual[o] = var_qual[v]; r->gt_qual[o] = gt_qual ? gt_qual[v] : float(cfg->max_qual);
                r->phase_set[o] = phase_set[v]; r->orig_gt[o] = orig_gt ? orig_gt[v] : VRL_GT_REF_REF;
            }
            continue;
        }
        I.n_realigned++;
        // variant qual is the cluster's minimum (from max_qual), phase set its first non-zero one (dist.cpp:2520-2535)
        float qual = float(cfg->max_qual);
        for (int v = b; v < e; v++) qual = std::min(qual, var_qual[v]);
        int32_t ps = 0;
        for (int v = b; v < e; v++) if (phase_set[v] != 0) { ps = phase_set[v]; break; }
        const float q_int = float(int32_t(qual));            // add_variants(..., int qual, ...)
        for (int64_t k = 0; k < nrec[size_t(c)]; k++, o++, rk++) {
            const RRec &R = recs[size_t(rk)];
            r->pos[o] = R.pos; r->rlen[o] = R.rlen; r->type[o] = R.type; r->ref_len[o] = R.ref_len; r->alt_len[o] = R.alt_len;
            memcpy(r->pool + po, rpool.data() + R.boff, size_t(R.ref_len) + size_t(R.alt_len));
            r->ref_off[o] = po; r->alt_off[o] = po + R.ref_len;
            po += R.ref_len + R.alt_len;
            r->var_qual[o] = q_int; r->gt_qual[o] = float(cfg->max_qual); r->phase_set[o] = ps; r->orig_gt[o] = VRL_GT_REF_REF;
        }
    }
    I.n_records = rk;
    left_shift(r, ctg_seq, ctg_len);
    I.ms_host = wall_ms() - t_host;
    I.ms_wall = wall_ms() - t_wall;
    r->info = I;
    *out = r;
    return VRL_OK;
}
