// pr_dist.hip -- the alignment-distance metrics (include/vcfdist_distance.h): edits_wrapper (dist.cpp:1908-2077) for an executed
// batch, on the device end to end.
//
// A job is (supercluster, query hap, quality threshold).  Steps, all on the library's stream:
//   k_dist_count   one thread per (supercluster, hap): the number of distinct thresholds {int(qual + 1)} u {max_qual + 2}
//                  (0 for a supercluster with a VPR_ST_ERR_* alignment); a scan gives the job offsets
//   k_dist_jobs    the jobs in ascending threshold order, their string lengths and pass-1 scratch sizes; the truth slot
//                  follows the device-resident sc_phase
//   k_dist_wave<false>  pass 1, one wavefront per job, lanes over diagonals: builds the reversed query / truth strings
//                  (generate_ptrs_strs with the quality filter) and runs wf_swg_align with a ring of max(x, o+e)+1 rows,
//                  for the score s and the exact size of the band-compacted history
//   k_dist_wave<true>   pass 2: the same recurrence, every row kept in a slice of the round arena
//   k_dist_back    one thread per job: wf_swg_backtrack over the history (swg_walk); the strings are reversed, so the backtrack emits
//                  the forward CIGAR in order and count_dist and the add_edits state machine run on the fly.  Launched
//                  twice: count (distance, record count, per-quality totals), then, after a scan, write.
//
// The recurrence, its band and the backtrack walk are shared with the realignment (pr_swg.h).
//
// Memory: the job tables live for the call; pass-1 scratch and pass-2 histories share one round arena.  Jobs run in
// rounds (pass 1: at most 4 GiB, pass 2: up to the plan, both capped by vpr_dist_config.round_bytes); a job larger than its
// round budget runs alone, a job larger than the memory plan (half the device's free memory) is marked VPR_DIST_ST_LIMIT.  Everything but what vpr_distance_download reads is
// released when the call returns; the rest goes with the next upload or execute.
#include "pr_host.h"
#include "pr_plan.h"
#include "pr_swg.h"
#include "../../include/vcfdist_distance.h"

#include <climits>

namespace {

using namespace swg;
const uint32_t DIST_ERR_BITS = VPR_ST_ERR_LIMIT | VPR_ST_ERR_NO_PTR | VPR_ST_ERR_UNFINISHED;

struct DTab {
    const int64_t *ctg_off;
    const uint8_t *ctg_seq;
    const int32_t *sc_ctg, *sc_beg, *sc_end;
    const int64_t *var_off[4];
    const int32_t *var_pos[4];
    const uint8_t *var_type[4];
    const float *var_qual[4];
    const int32_t *ref_len[4], *alt_len[4];
    const int64_t *alt_off[4];
    const uint8_t *pool[4];
    const int32_t *sc_phase;
    const uint32_t *aln_status;
    int32_t n_sc, max_qual;
};

struct DJob { int32_t sc, hap, minq, maxq, q_len, t_len, tslot, pad; };
struct DEdit { int32_t sc, pos, len, minq, maxq; uint8_t hap, type, pad[2]; };

// the threshold a variant adds to the set (dist.cpp:2014: float + 1 stored in a std::set<int>)
__device__ inline int qual_key(float q) {
    const float k = q + 1.0f;
    return k >= 2147483520.0f ? INT_MAX - 1 : k > -2147483520.0f ? int(k) : INT_MIN + 1;   // (NaN and the extremes stay defined)
}

__device__ inline bool sc_bad(const DTab &T, int sc) {
    uint32_t st = 0;
    for (int k = 0; k < 4; k++) st |= T.aln_status[4 * sc + k];
    return (st & DIST_ERR_BITS) != 0;
}

// generate_ptrs_strs' string (dist.cpp:145-242) of hap slot `slot` over the supercluster's region, variants with
// qual >= minq only: emit(src, n) for every piece in order.  false: the walk went backwards (overlapping variants,
// which the reference cannot process either).
template <typename F>
__device__ bool gen_walk(const DTab &T, int slot, int sc, float minq, F emit) {
    const int ctg = T.sc_ctg[sc];
    const uint8_t *fa = T.ctg_seq + T.ctg_off[ctg];
    const int64_t ctg_len = T.ctg_off[ctg + 1] - T.ctg_off[ctg];
    const int beg = T.sc_beg[sc];
    const int end = int(min(int64_t(T.sc_end[sc]), ctg_len - 1));
    int64_t v = T.var_off[slot][sc];
    const int64_t ve = T.var_off[slot][sc + 1];
    for (int pos = beg; pos <= end;) {
        if (v < ve && pos == T.var_pos[slot][v]) {
            if (T.var_qual[slot][v] >= minq) {
                const int type = T.var_type[slot][v];
                if (type == VPR_TYPE_INS) emit(T.pool[slot] + T.alt_off[slot][v], T.alt_len[slot][v]);
                else if (type == VPR_TYPE_DEL) pos += T.ref_len[slot][v];
                else { emit(T.pool[slot] + T.alt_off[slot][v], 1); pos++; }
            }
            v++;
        } else {
            const int stop = v < ve ? T.var_pos[slot][v] : end + 1;
            if (stop < pos || stop > ctg_len) return false;
            emit(fa + pos, stop - pos);
            pos = stop;
        }
    }
    return true;
}

__device__ int gen_len(const DTab &T, int slot, int sc, float minq, bool *ok) {
    int n = 0;
    *ok = gen_walk(T, slot, sc, minq, [&](const uint8_t *, int k) { n += k; });
    return n;
}

// the thresholds of (supercluster, hap) in ascending order, {int(qual + 1)} u {max_qual + 2}: fn(prev_qual, qual) per job.
// (k_dist_count and k_dist_jobs enumerate with this one loop, so the job counts and the jobs written agree whatever the qualities)
template <typename F>
__device__ void for_thresholds(const DTab &T, int hap, int sc, F fn) {
    const int64_t b = T.var_off[hap][sc], e = T.var_off[hap][sc + 1];
    const int top = T.max_qual + 2;
    int prev = 0, cur = INT_MIN;
    for (;;) {                  // the smallest key above the last one
        int next = top > cur ? top : INT_MAX;
        for (int64_t v = b; v < e; v++) {
            const int k = qual_key(T.var_qual[hap][v]);
            if (k > cur && k < next) next = k;
        }
        if (next == INT_MAX) break;
        fn(prev, next);
        prev = cur = next;
    }
}

__global__ void k_dist_count(DTab T, int64_t *cnt) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= 2 * T.n_sc) return;
    const int sc = i >> 1, hap = i & 1;
    int64_t n = 0;
    if (!sc_bad(T, sc)) for_thresholds(T, hap, sc, [&](int, int) { n++; });
    cnt[i] = n;
}

__global__ void k_dist_jobs(DTab T, const int64_t *job_off, DJob *jobs, int64_t *need, uint8_t *status, int P) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= 2 * T.n_sc) return;
    const int sc = i >> 1, hap = i & 1;
    if (sc_bad(T, sc)) return;
    const int tslot = 2 + (T.sc_phase[sc] == VPR_PHASE_SWAP ? 1 - hap : hap);
    bool tok;
    const int t_len = gen_len(T, tslot, sc, 0.0f, &tok);
    int64_t j = job_off[i];
    for_thresholds(T, hap, sc, [&](int prev, int next) {
        bool qok;
        const int q_len = gen_len(T, hap, sc, float(prev), &qok);
        DJob J;
        J.sc = sc; J.hap = hap; J.minq = prev; J.maxq = next; J.q_len = q_len; J.t_len = t_len; J.tslot = tslot; J.pad = 0;
        jobs[j] = J;
        const bool ok = tok && qok && q_len > 0 && t_len > 0;
        status[j] = ok ? 0 : VPR_DIST_ST_ERROR;
        need[j] = ok ? need1(q_len, t_len, P) : 0;
        j++;
    });
}

// the job's strings, reversed (dist.cpp:2047-2048), lanes writing each piece side by side
__device__ void load_reversed(const DTab &T, const DJob &J, uint8_t *qs, uint8_t *ts, int lane) {
    int n = 0;
    gen_walk(T, J.hap, J.sc, float(J.minq), [&](const uint8_t *src, int k) {
        for (int c = lane; c < k; c += 64) qs[J.q_len - 1 - (n + c)] = src[c];
        n += k;
    });
    n = 0;
    gen_walk(T, J.tslot, J.sc, 0.0f, [&](const uint8_t *src, int k) {
        for (int c = lane; c < k; c += 64) ts[J.t_len - 1 - (n + c)] = src[c];
        n += k;
    });
}

// pass 1 (HIST = false) / pass 2 (HIST = true) of one job per wavefront (swg_wave, pr_swg.h).  Pass 1 writes the score and the bytes
// pass 2 will need; pass 2 writes the history into the slice its caller sized from them.
template <bool HIST>
__global__ void __launch_bounds__(64) k_dist_wave(DTab T, const DJob *__restrict__ jobs, int64_t j0, int64_t n,
                                                   const int64_t *__restrict__ slice, int64_t slice_base, uint8_t *arena,
                                                   uint8_t *status, int32_t *score, int64_t *need2_out, int64_t *cells_out, DPen pen) {
    const int64_t j = j0 + int64_t(blockIdx.x);
    if (int64_t(blockIdx.x) >= n) return;
    if (status[j]) return;
    const DJob J = jobs[j];
    const WaveOut W = swg_wave<HIST>(J.q_len, J.t_len, pen, arena + (slice[j] - slice_base), HIST ? score[j] : 0,
                                     HIST ? cells_out[j] : 0, [&](uint8_t *qs, uint8_t *ts, int lane) { load_reversed(T, J, qs, ts, lane); });
    if (threadIdx.x != 0) return;
    if (W.failed) { status[j] |= VPR_DIST_ST_ERROR; return; }
    if (!HIST) {
        score[j] = W.s;
        cells_out[j] = W.cells;
        need2_out[j] = need2(J.q_len, J.t_len, W.s, W.cells);
    }
}

// add_edits (edit.cpp:4-78) as a state machine over the CIGAR's steps (a MAT / SUB step is the reference's two CIGAR
// entries, INS / DEL one): a run is recorded when the next run starts, a SUB run one record per base -- so the run still
// open at the end is never recorded
struct EditSM {
    int last = DP_MAT, len = 0, pos;
    template <typename R>
    __device__ void step(int type, R rec) {
        if (type != last) {
            if (last == DP_SUB) rec(pos - 1, VPR_TYPE_SUB, 1);
            else if (last == DP_INS) rec(pos, VPR_TYPE_INS, len);
            else if (last == DP_DEL) rec(pos - len, VPR_TYPE_DEL, len);
            last = type; len = 1;
        } else {
            if (type == DP_SUB) rec(pos - 1, VPR_TYPE_SUB, 1);
            len++;
        }
        if (type != DP_INS) pos++;
    }
};

// wf_swg_backtrack (dist.cpp:2625-2757) of one job per thread.  WRITE = false: distance, record count and the per-quality
// totals (a difference array of max_qual + 3 words); WRITE = true: the records at the offsets the scan gave.
template <bool WRITE>
__global__ void k_dist_back(DTab T, const DJob *__restrict__ jobs, int64_t j0, int64_t n, const int64_t *__restrict__ slice,
                            int64_t slice_base, const uint8_t *arena, uint8_t *status, const int32_t *score, const int64_t *cells_in,
                            int32_t *dist_out, int64_t *n_rec, const int64_t *rec_off, int64_t rec_base, DEdit *rec_out,
                            unsigned long long *qdiff, DPen pen) {
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t j = j0 + k;
    if (status[j]) { if (!WRITE) { dist_out[j] = 0; n_rec[k] = 0; } return; }
    const DJob J = jobs[j];
    const int q = J.q_len, t = J.t_len;
    const uint8_t *base = arena + (slice[j] - slice_base);
    int64_t nr = 0, out = WRITE ? rec_off[k] - rec_base : 0;
    auto rec = [&](int pos, int type, int len) {
        if (WRITE) {
            DEdit E;
            E.sc = J.sc; E.pos = pos; E.len = len; E.minq = J.minq; E.maxq = J.maxq; E.hap = uint8_t(J.hap); E.type = uint8_t(type);
            E.pad[0] = E.pad[1] = 0;
            rec_out[out + nr] = E;
        }
        nr++;
    };
    EditSM sm;
    sm.pos = T.sc_beg[J.sc];
    int dist = 0;
    const bool bad = !swg_walk(base, q, t, score[j], cells_in[j], pen, [&](int type, int, int) { dist += type != DP_MAT; sm.step(type, rec); });
    if (WRITE) return;
    if (bad) { status[j] |= VPR_DIST_ST_ERROR; dist_out[j] = 0; n_rec[k] = 0; return; }
    dist_out[j] = dist;
    n_rec[k] = nr;
    // all_qual_dists[q] += dist for q in [prev_qual, qual) (dist.cpp:2059-2063), as a difference array
    const int top = T.max_qual + 2;
    const int lo = max(J.minq, 0), hi = min(J.maxq, top);
    if (dist && lo < hi) {
        atomicAdd(&qdiff[lo], (unsigned long long)(int64_t)dist);
        atomicAdd(&qdiff[hi], (unsigned long long)(-(int64_t)dist));
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct DistState {
    DevBuf<uint8_t> in_blk;                                 // the uploaded tables
    DevBuf<DJob> jobs;                                      // job tables (grown on demand)
    DevBuf<int64_t> need1, need2, cells, slice, nrec, recoff;
    DevBuf<int32_t> score, dist;
    DevBuf<uint8_t> status;
    DevBuf<int64_t> cnt, cnt_off;
    DevBuf<uint8_t> scan_tmp;
    DevBuf<unsigned long long> qdiff;
    DevBuf<uint8_t> arena;
    DevBuf<DEdit> edits;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int32_t max_qual = 0;
    bool valid = false;
    vpr_dist_info info;
};

namespace {

int scan_i64(vpr_handle *h, DistState *D, const int64_t *in, int64_t *out, size_t n) {
    size_t need = 0;
    if (vplan_exclusive_scan_i64(nullptr, &need, in, out, n, h->stream)) return fail(h, VPR_ERR_DEVICE, "vpr_distance: scan sizing failed");
    if (int rc = D->scan_tmp.reserve(h, need, "vpr_distance: cannot allocate %zu bytes on the device (scan workspace)")) return rc;
    if (vplan_exclusive_scan_i64(D->scan_tmp.p, &need, in, out, n, h->stream)) return fail(h, VPR_ERR_DEVICE, "vpr_distance: scan failed");
    return VPR_OK;
}

double ev_ms(DistState *D) {
    float ms = 0;
    (void)hipEventSynchronize(D->ev[1]);
    (void)hipEventElapsedTime(&ms, D->ev[0], D->ev[1]);
    return ms;
}

}  // namespace

// the buffers only a vpr_distance call itself uses (tables, pass scratch, round arena): released when it returns, so that the
// memory the next vpr_execute plans with is not held by the distance step.  What vpr_distance_download reads stays.
void dist_release_work(vpr_handle *h) {
    DistState *D = h->dist;
    if (D) dev_release(h, D->in_blk, D->need1, D->need2, D->cells, D->slice, D->nrec, D->recoff, D->score, D->cnt, D->cnt_off, D->scan_tmp, D->arena);
}

// everything of the distance step, results included: called by vpr_destroy, by every upload (free_batch) and at the start of
// vpr_execute, so that vpr_distance_download / vpr_distance_info never return an earlier batch's or execute's results
void dist_free(vpr_handle *h) {
    DistState *D = h->dist;
    if (!D) return;
    dist_release_work(h);
    dev_release(h, D->jobs, D->dist, D->status, D->qdiff, D->edits);
    for (int k = 0; k < 2; k++) if (D->ev[k]) (void)hipEventDestroy(D->ev[k]);
    delete D;
    h->dist = nullptr;
}

extern "C" int vpr_distance(vpr_handle *h, const vpr_variants *v, const vpr_dist_config *cfg) {
    if (!h) return VPR_ERR_ARG;
    if (!v || !cfg) return fail(h, VPR_ERR_ARG, "vpr_distance: null argument");
    if (!h->executed) return fail(h, VPR_ERR_ARG, "vpr_distance: no batch has been executed");
    if (v->n_sc != h->n_sc) return fail(h, VPR_ERR_ARG, "vpr_distance: %d superclusters given, the executed batch has %d", v->n_sc, h->n_sc);
    if (cfg->eval_sub < 1 || cfg->eval_open < 0 || cfg->eval_extend < 1 || cfg->max_qual < 0 || cfg->max_qual > (1 << 24))
        return fail(h, VPR_ERR_ARG, "vpr_distance: eval_sub and eval_extend must be at least 1, eval_open and max_qual non-negative");
    if (v->n_sc > 0 && (!v->ctg_off || !v->ctg_seq || !v->sc_ctg || !v->sc_beg || !v->sc_end))
        return fail(h, VPR_ERR_ARG, "vpr_distance: null table");
    const double t_wall = wall_ms();
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->dist) {
        h->dist = new DistState();
        HIPCHK(h, hipEventCreate(&h->dist->ev[0]));
        HIPCHK(h, hipEventCreate(&h->dist->ev[1]));
    }
    DistState *D = h->dist;
    D->valid = false;
    struct Release { vpr_handle *h; ~Release() { (void)hipStreamSynchronize(h->stream); dist_release_work(h); } } release{h};
    memset(&D->info, 0, sizeof(D->info));
    vpr_dist_info &I = D->info;
    const int64_t n_sc = v->n_sc;
    const DPen pen{cfg->eval_sub, cfg->eval_open, cfg->eval_extend};
    const int P = std::max(pen.x, pen.o + pen.e) + 1;
    D->max_qual = cfg->max_qual;
    const int nqd = cfg->max_qual + 3;
    if (int rc = D->qdiff.reserve(h, size_t(nqd), "vpr_distance: cannot allocate %zu bytes on the device (quality totals)")) return rc;
    HIPCHK(h, hipMemsetAsync(D->qdiff.p, 0, sizeof(unsigned long long) * nqd, h->stream));
    if (n_sc == 0) { D->valid = true; I.ms_wall = wall_ms() - t_wall; return VPR_OK; }

    // ---- the tables the jobs read, one block (the resident Level A arrays hold the unfiltered strings only)
    const double t_up = wall_ms();
    struct Piece { const void *src; size_t bytes; size_t at; };
    std::vector<Piece> pieces;
    size_t total = 0;
    auto add = [&](const void *src, size_t bytes) { pieces.push_back({src, bytes, total}); total += (bytes + 255) & ~size_t(255); return pieces.size() - 1; };
    const size_t i_ctg_off = add(v->ctg_off, sizeof(int64_t) * (size_t(v->n_ctg) + 1));
    const size_t i_ctg_seq = add(v->ctg_seq, size_t(v->ctg_off[v->n_ctg]));
    const size_t i_sc_ctg = add(v->sc_ctg, 4 * size_t(n_sc)), i_beg = add(v->sc_beg, 4 * size_t(n_sc)), i_end = add(v->sc_end, 4 * size_t(n_sc));
    size_t i_var[4][8];
    for (int s = 0; s < 4; s++) {
        if (!v->var_off[s]) return fail(h, VPR_ERR_ARG, "vpr_distance: null var_off");
        const int64_t nv = v->var_off[s][n_sc];
        int64_t pool = 1;
        for (int64_t k = 0; k < nv; k++) pool = std::max(pool, v->var_alt_off[s][k] + v->var_alt_len[s][k]);
        i_var[s][0] = add(v->var_off[s], 8 * (size_t(n_sc) + 1));
        i_var[s][1] = add(v->var_pos[s], 4 * size_t(nv));
        i_var[s][2] = add(v->var_type[s], size_t(nv));
        i_var[s][3] = add(v->var_qual[s], 4 * size_t(nv));
        i_var[s][4] = add(v->var_ref_len[s], 4 * size_t(nv));
        i_var[s][5] = add(v->var_alt_len[s], 4 * size_t(nv));
        i_var[s][6] = add(v->var_alt_off[s], 8 * size_t(nv));
        i_var[s][7] = add(v->allele_pool[s], size_t(nv ? pool : 0));
    }
    if (int rc = D->in_blk.reserve(h, total, "vpr_distance: cannot allocate %zu bytes on the device (input tables)")) return rc;
    for (const Piece &p : pieces)
        if (p.bytes && p.src) HIPCHK(h, hipMemcpyAsync(D->in_blk.p + p.at, p.src, p.bytes, hipMemcpyHostToDevice, h->stream));
    I.input_bytes = int64_t(total);
    auto at = [&](size_t i) { return D->in_blk.p + pieces[i].at; };
    DTab T;
    T.ctg_off = reinterpret_cast<const int64_t *>(at(i_ctg_off));
    T.ctg_seq = at(i_ctg_seq);
    T.sc_ctg = reinterpret_cast<const int32_t *>(at(i_sc_ctg));
    T.sc_beg = reinterpret_cast<const int32_t *>(at(i_beg));
    T.sc_end = reinterpret_cast<const int32_t *>(at(i_end));
    for (int s = 0; s < 4; s++) {
        T.var_off[s] = reinterpret_cast<const int64_t *>(at(i_var[s][0]));
        T.var_pos[s] = reinterpret_cast<const int32_t *>(at(i_var[s][1]));
        T.var_type[s] = at(i_var[s][2]);
        T.var_qual[s] = reinterpret_cast<const float *>(at(i_var[s][3]));
        T.ref_len[s] = reinterpret_cast<const int32_t *>(at(i_var[s][4]));
        T.alt_len[s] = reinterpret_cast<const int32_t *>(at(i_var[s][5]));
        T.alt_off[s] = reinterpret_cast<const int64_t *>(at(i_var[s][6]));
        T.pool[s] = at(i_var[s][7]);
    }
    T.sc_phase = h->dR.sc_phase;
    T.aln_status = h->dR.aln_status;
    T.n_sc = int32_t(n_sc);
    T.max_qual = cfg->max_qual;
    I.ms_upload = wall_ms() - t_up;

    // ---- the jobs
    const size_t n_hs = size_t(2 * n_sc);
    if (int rc = D->cnt.reserve(h, n_hs + 1, "vpr_distance: cannot allocate %zu bytes on the device (job counts)")) return rc;
    if (int rc = D->cnt_off.reserve(h, n_hs + 1, "vpr_distance: cannot allocate %zu bytes on the device (job offsets)")) return rc;
    HIPCHK(h, hipEventRecord(D->ev[0], h->stream));
    hipLaunchKernelGGL(k_dist_count, dim3(unsigned((n_hs + 255) / 256)), dim3(256), 0, h->stream, T, D->cnt.p);
    HIPCHK(h, hipMemsetAsync(D->cnt.p + n_hs, 0, sizeof(int64_t), h->stream));
    if (int rc = scan_i64(h, D, D->cnt.p, D->cnt_off.p, n_hs + 1)) return rc;
    int64_t n_jobs = 0;
    HIPCHK(h, hipMemcpyAsync(&n_jobs, D->cnt_off.p + n_hs, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    I.n_jobs = n_jobs;
    {   // the per-job tables: one entry more than the jobs, at least 256 bytes each
        const size_t nj = size_t(std::max<int64_t>(n_jobs, 1)) + 1;
        auto table = [&](auto &b) { return b.reserve(h, std::max(nj, 256 / sizeof(*b.p)), "") != VPR_OK; };
        if (table(D->jobs) || table(D->need1) || table(D->need2) || table(D->cells) || table(D->slice) || table(D->nrec) ||
            table(D->recoff) || table(D->score) || table(D->dist) || table(D->status))
            return fail(h, VPR_ERR_NOMEM, "vpr_distance: cannot allocate the tables of %lld jobs", (long long)n_jobs);
    }
    if (n_jobs > 0)
        hipLaunchKernelGGL(k_dist_jobs, dim3(unsigned((n_hs + 255) / 256)), dim3(256), 0, h->stream, T, D->cnt_off.p, D->jobs.p, D->need1.p,
                           D->status.p, P);
    HIPCHK(h, hipEventRecord(D->ev[1], h->stream));
    HIPCHK(h, hipGetLastError());
    I.ms_jobs = ev_ms(D);
    std::vector<int64_t> n1(static_cast<size_t>(n_jobs));
    std::vector<uint8_t> st(static_cast<size_t>(n_jobs));
    if (n_jobs) {
        HIPCHK(h, hipMemcpyAsync(n1.data(), D->need1.p, 8 * size_t(n_jobs), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(st.data(), D->status.p, size_t(n_jobs), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, x_sync(h, h->stream, SITE));
    }

    // ---- memory plan: half of what the device has free (by the process's books) for one job; the round budget is that or the
    // caller's cap
    size_t fr = 0, tt = 0;
    HIPCHK(h, hipMemGetInfo(&fr, &tt));
    const int64_t plan = std::max<int64_t>(books_free(int64_t(fr), int64_t(tt)) / 2, int64_t(1) << 20);
    // Pass-1 rounds of at most 4 GiB (a whole-genome batch's full-width rings came to 17 GB at once; in four rounds the call took
    // 183 -> 220-240 ms).  Pass-2 rounds take up to the plan: a history round is as long as its longest job, and with 4 GiB the SV-sized jobs
    // of joint_synth ran in 31 rounds instead of 2 (7 s -> 62 s).  round_bytes caps both.
    const int64_t round_cap1 = std::min<int64_t>(cfg->round_bytes > 0 ? cfg->round_bytes : int64_t(4) << 30, plan);
    const int64_t round_cap2 = cfg->round_bytes > 0 ? std::min<int64_t>(cfg->round_bytes, plan) : plan;
    I.plan_bytes = plan;
    int64_t n_edits = 0, got = 0;
    // the backtrack of a sub-round: count, scan, room for the records (the buffer doubles and keeps what it holds), write
    auto back = [&](int64_t c, int64_t m, uint8_t *arena) -> int {
        const unsigned gb = unsigned((m + 63) / 64);
        hipLaunchKernelGGL(k_dist_back<false>, dim3(gb), dim3(64), 0, h->stream, T, D->jobs.p, c, m, D->slice.p, int64_t(0), arena,
                           D->status.p, D->score.p, D->cells.p, D->dist.p, D->nrec.p, D->recoff.p, int64_t(0), D->edits.p, D->qdiff.p, pen);
        HIPCHK(h, hipMemsetAsync(D->nrec.p + m, 0, sizeof(int64_t), h->stream));
        if (int rc = scan_i64(h, D, D->nrec.p, D->recoff.p, size_t(m) + 1)) return rc;
        HIPCHK(h, hipMemcpyAsync(&got, D->recoff.p + m, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, x_sync(h, h->stream, SITE));
        if (size_t(n_edits + got) > D->edits.cap) {
            const size_t cap = std::max(D->edits.cap * 2, std::max<size_t>(size_t(n_edits + got), 1024));
            if (int rc = D->edits.reserve(h, cap, "", size_t(n_edits)))
                return rc == VPR_ERR_NOMEM ? fail(h, rc, "vpr_distance: cannot allocate %lld edit records", (long long)cap) : rc;
        }
        if (got)
            hipLaunchKernelGGL(k_dist_back<true>, dim3(gb), dim3(64), 0, h->stream, T, D->jobs.p, c, m, D->slice.p, int64_t(0), arena,
                               D->status.p, D->score.p, D->cells.p, D->dist.p, D->nrec.p, D->recoff.p, -n_edits, D->edits.p, D->qdiff.p, pen);
        return VPR_OK;
    };
    int rc_back = VPR_OK;
    swg::Rounds R{h->stream, {D->ev[0], D->ev[1]}, plan, round_cap1, round_cap2, VPR_DIST_ST_LIMIT, D->slice.p, D->status.p, D->need2.p};
    const int rr = R.run(
        n1, st, [&] { return x_sync(h, h->stream, SITE); },
        [&](int64_t bytes) { return D->arena.reserve(h, size_t(bytes), "vpr_distance: cannot allocate a round arena of %zu bytes") ? nullptr : D->arena.p; },
        [&](bool hist, int64_t a, int64_t n, uint8_t *arena) {
            if (hist)
                hipLaunchKernelGGL(k_dist_wave<true>, dim3(unsigned(n)), dim3(64), 0, h->stream, T, D->jobs.p, a, n, D->slice.p, int64_t(0), arena,
                                   D->status.p, D->score.p, D->need2.p, D->cells.p, pen);
            else
                hipLaunchKernelGGL(k_dist_wave<false>, dim3(unsigned(n)), dim3(64), 0, h->stream, T, D->jobs.p, a, n, D->slice.p, int64_t(0), arena,
                                   D->status.p, D->score.p, D->need2.p, D->cells.p, pen);
        },
        [&](int64_t c, int64_t m, uint8_t *arena) { return (rc_back = back(c, m, arena)) ? int(ROUNDS_DEVICE) : int(ROUNDS_OK); },
        [&](int64_t, int64_t) { n_edits += got; return int(ROUNDS_OK); });
    I.n_rounds = R.n_rounds; I.n_hist_rounds = R.n_hist_rounds; I.arena_bytes = R.arena_bytes;
    if (rc_back) return rc_back;
    if (rr == ROUNDS_NOMEM) return VPR_ERR_NOMEM;           // (the message is the arena's)
    if (rr) return fail(h, VPR_ERR_DEVICE, "vpr_distance: %s failed: %s", R.what, hipGetErrorString(R.err));
    // cells of the histories, for the statistics
    if (n_jobs) {
        std::vector<int64_t> cl(static_cast<size_t>(n_jobs));
        HIPCHK(h, hipMemcpyAsync(cl.data(), D->cells.p, 8 * size_t(n_jobs), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, x_sync(h, h->stream, SITE));
        for (int64_t k = 0; k < n_jobs; k++) if (!st[size_t(k)]) I.history_cells += cl[size_t(k)];
        for (uint8_t s : st) { I.n_limit += (s & VPR_DIST_ST_LIMIT) != 0; I.n_error += (s & VPR_DIST_ST_ERROR) != 0; }
        // jobs that never ran keep no distance
        HIPCHK(h, hipMemcpyAsync(D->status.p, st.data(), size_t(n_jobs), hipMemcpyHostToDevice, h->stream));
    }
    I.n_edits = n_edits;
    I.ms_score = R.ms_score; I.ms_hist = R.ms_hist; I.ms_back = R.ms_back;
    HIPCHK(h, x_sync(h, h->stream, SITE));
    I.ms_wall = wall_ms() - t_wall;
    D->valid = true;
    return VPR_OK;
}

extern "C" int vpr_distance_info(const vpr_handle *h, vpr_dist_info *out) {
    if (!h || !out || !h->dist || !h->dist->valid) return VPR_ERR_ARG;
    *out = h->dist->info;
    return VPR_OK;
}

extern "C" int vpr_distance_download(vpr_handle *h, vpr_dist_results *r) {
    if (!h) return VPR_ERR_ARG;
    if (!r || !h->dist || !h->dist->valid) return fail(h, VPR_ERR_ARG, "vpr_distance_download: no vpr_distance results");
    DistState *D = h->dist;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t nj = D->info.n_jobs, ne = D->info.n_edits;
    const int nq = D->max_qual + 2;
    std::vector<DJob> jobs(static_cast<size_t>(nj));
    std::vector<int32_t> dist(static_cast<size_t>(nj));
    std::vector<uint8_t> st(static_cast<size_t>(nj));
    std::vector<DEdit> ed(static_cast<size_t>(ne));
    std::vector<unsigned long long> qd(size_t(nq) + 1);
    if (nj) {
        HIPCHK(h, hipMemcpyAsync(jobs.data(), D->jobs.p, sizeof(DJob) * size_t(nj), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(dist.data(), D->dist.p, 4 * size_t(nj), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(st.data(), D->status.p, size_t(nj), hipMemcpyDeviceToHost, h->stream));
    }
    if (ne) HIPCHK(h, hipMemcpyAsync(ed.data(), D->edits.p, sizeof(DEdit) * size_t(ne), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(qd.data(), D->qdiff.p, sizeof(unsigned long long) * (size_t(nq) + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    for (int64_t k = 0; k < nj; k++) {
        const DJob &J = jobs[size_t(k)];
        if (r->job_sc) r->job_sc[k] = J.sc;
        if (r->job_hap) r->job_hap[k] = uint8_t(J.hap);
        if (r->job_min_qual) r->job_min_qual[k] = J.minq;
        if (r->job_max_qual) r->job_max_qual[k] = J.maxq;
        if (r->job_dist) r->job_dist[k] = st[size_t(k)] ? 0 : dist[size_t(k)];
        if (r->job_status) r->job_status[k] = st[size_t(k)];
    }
    if (r->qual_dists) {
        int64_t run = 0;
        for (int q = 0; q < nq; q++) { run += int64_t(qd[size_t(q)]); r->qual_dists[q] = run; }
    }
    for (int64_t k = 0; k < ne; k++) {
        const DEdit &E = ed[size_t(k)];
        if (r->edit_sc) r->edit_sc[k] = E.sc;
        if (r->edit_hap) r->edit_hap[k] = E.hap;
        if (r->edit_pos) r->edit_pos[k] = E.pos;
        if (r->edit_type) r->edit_type[k] = E.type;
        if (r->edit_len) r->edit_len[k] = E.len;
        if (r->edit_min_qual) r->edit_min_qual[k] = E.minq;
        if (r->edit_max_qual) r->edit_max_qual[k] = E.maxq;
    }
    return VPR_OK;
}
