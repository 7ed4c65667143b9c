// pr_strata.hip -- the region-stratified precision/recall counters (include/vcfdist_strata.h): one evaluation, cut by region
// afterwards.  k_strata_mask gives every variant a bit per stratum (the membership rule is the host's vio_bed_contains ==
// VIO_BED_INSIDE, vcf_io.cpp, which follows bedData::contains, bed.cpp:73-121); k_pr_hist_strata counts a variant's bin
// (pr_counts.h) into every stratum whose bit is set.  The host fold of a histogram and the front and back of a counters call
// are the ones of pr_collect.hip.
#include "pr_host.h"
#include "pr_counts.h"
#include "../../include/vcfdist_strata.h"

struct StrataState {
    int32_t n_strata = 0, n_words = 0;
    int64_t n_var[VPR_HAPS] = {0, 0, 0, 0};
    DevBuf<uint64_t> words[VPR_HAPS];                                   // word-major: [n_words][n_var[slot]]
    DevBuf<unsigned long long> hist;                                    // [n_strata][2][3 classes][3][nq + 1]
    bool valid = false;
    // device time of the last k_strata_mask launches / k_pr_hist_strata launches (vpr_strata_timing)
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_mask = 0, ms_hist = 0;
};

namespace {

const int TYPE_INS = 2;               // VPR_TYPE_INS
// LDS a workgroup of k_pr_hist_strata may ask for: four of them fit beside each other in a compute unit's 160 KiB
const size_t HIST_LDS_BUDGET = 40 * 1024;

// strata of one workgroup of k_pr_hist_strata: the largest power of two up to 64 (a chunk then never straddles a
// membership word) whose privatised bins fit the budget; one stratum when even that does not
int hist_chunk(int nq) {
    const size_t per = size_t(9) * size_t(nq + 1) * 4;
    int c = 64;
    while (c > 1 && size_t(c) * per > HIST_LDS_BUDGET) c >>= 1;
    return c;
}

}  // namespace

extern "C" {

// One lane per variant, blockIdx.y the 64-stratum word.  The lane walks the word's strata, does the two bisections of
// vio_bed_contains on the stratum's row of its contig and assembles the word in registers: one plain 8-byte store, coalesced
// in the word-major layout.  Consecutive lanes hold consecutive positions of one slot, so the top levels of every
// bisection are wave-uniform and the loads hit the same lines.
__global__ void __launch_bounds__(256) k_strata_mask(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                                                     const int32_t *__restrict__ sc_ctg, const int32_t *__restrict__ var_pos,
                                                     const int32_t *__restrict__ var_ref_len, const uint8_t *__restrict__ var_type,
                                                     const int64_t *__restrict__ iv_off, const int32_t *__restrict__ iv_start,
                                                     const int32_t *__restrict__ iv_stop, int n_strata, int n_ctg,
                                                     uint64_t *__restrict__ words /* [n_words][n_var] */) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n_var) return;
    const int w = blockIdx.y;
    const int ctg = sc_ctg[sc_of_var(var_off, n_sc, v)];
    const int32_t start = var_pos[v], stop = start + var_ref_len[v];
    const bool ins = var_type[v] == TYPE_INS;
    const int k_end = min(n_strata, (w + 1) * 64);
    uint64_t word = 0;
    for (int k = w * 64; k < k_end; k++) {
        const int64_t row = int64_t(k) * n_ctg + ctg;
        const int64_t r0 = iv_off[row];
        const int n = int(iv_off[row + 1] - r0);
        if (n == 0) continue;                                                  // OFFCTG
        const int32_t *__restrict__ st = iv_start + r0, *__restrict__ sp = iv_stop + r0;
        if (stop <= st[0] || start >= sp[n - 1]) continue;                     // OUTSIDE
        int lo = 0, hi = n;              // a = upper_bound(starts, start) - 1
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (st[mid] <= start) lo = mid + 1; else hi = mid; }
        const int a = lo - 1;
        lo = 0; hi = n;                  // b = lower_bound(stops, stop)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (sp[mid] < stop) lo = mid + 1; else hi = mid; }
        const int b = lo;
        // INSIDE: one region holds the whole span, and an insertion does not sit on the region's last base
        if (a >= 0 && b < n && a == b && !(ins && start == sp[b] - 1)) word |= uint64_t(1) << (k & 63);
    }
    words[size_t(w) * size_t(n_var) + size_t(v)] = word;
}

// k_pr_hist with a stratum dimension: blockIdx.y is a chunk of n_chunk strata (a power of two up to 64, so the chunk's bits
// lie in one membership word), whose 9 x (nq + 1) bins per stratum are privatised in LDS and flushed once with 64-bit
// global atomics.  A lane whose bits of the chunk are all zero does nothing.
__global__ void __launch_bounds__(256) k_pr_hist_strata(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                                 const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                                 const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, int callset, int min_qual,
                                 int max_qual, const uint64_t *__restrict__ words, int n_strata, int n_chunk,
                                 unsigned long long *__restrict__ hist /* [n_strata][2][3 classes][3][nq + 1] */) {
    extern __shared__ unsigned int blk[];      // [n_chunk][3][3][nq + 1]
    const int nq = max_qual - min_qual + 1, nb = 9 * (nq + 1);
    const int k0 = blockIdx.y * n_chunk, nk = min(n_chunk, n_strata - k0);
    for (int k = threadIdx.x; k < nk * nb; k += blockDim.x) blk[k] = 0;
    __syncthreads();
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n_var) {
        uint64_t bits = words[size_t(k0 >> 6) * size_t(n_var) + size_t(v)] >> (k0 & 63);
        if (nk < 64) bits &= (uint64_t(1) << nk) - 1;
        if (bits) {
            int b = 0;
            const int row = pr_count_row(sc_of_var(var_off, n_sc, v), v, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, cls,
                                         min_qual, nq, &b);
            const int bin = row * (nq + 1) + b;
            while (row >= 0 && bits) {
                const int j = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                atomicAdd(&blk[j * nb + bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nk * nb; k += blockDim.x)
        if (blk[k]) atomicAdd(&hist[(size_t(k0 + k / nb) * 2 + size_t(callset)) * nb + size_t(k % nb)], (unsigned long long)blk[k]);
}

}  // extern "C"

namespace {

double ev_ms(const StrataState *S) {     // (both events have completed: the caller has synchronised the stream)
    float ms = 0;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]);
    return ms;
}

void release_words(vpr_handle *h, StrataState *S) {
    for (int s = 0; s < VPR_HAPS; s++) { S->words[s].release(h); S->n_var[s] = 0; }
    S->valid = false;
}

// the state with room for n_words words of n_var[s] variants per slot (earlier words are released)
int strata_prepare(vpr_handle *h, int32_t n_strata, const int64_t n_var[VPR_HAPS]) {
    if (!h->strata) h->strata = new StrataState();
    StrataState *S = h->strata;
    for (int k = 0; k < 2; k++) if (!S->ev[k]) HIPCHK(h, hipEventCreate(&S->ev[k]));
    release_words(h, S);
    S->ms_mask = S->ms_hist = 0;
    S->n_strata = n_strata; S->n_words = (n_strata + 63) / 64;
    for (int s = 0; s < VPR_HAPS; s++) {
        const size_t n = std::max<size_t>(size_t(S->n_words) * size_t(n_var[s]), 32);
        if (int rc = S->words[s].reserve(h, n, "stratum membership words: cannot allocate %zu bytes on the device")) {
            release_words(h, S);
            return rc;
        }
        S->n_var[s] = n_var[s];
    }
    return VPR_OK;
}

int strata_counts_impl(vpr_handle *h, void *comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                       int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!h || !counts || max_qual < min_qual) return VPR_ERR_ARG;
    if (int rc = pr_counts_begin(h, "vpr_pr_counts_strata", comm)) return rc;
    int32_t n_strata = 0;
    const uint64_t *words[VPR_HAPS];
    if (int rc = strata_view(h, "vpr_pr_counts_strata", &n_strata, words)) return rc;
    StrataState *S = h->strata;
    const int nq = max_qual - min_qual + 1;
    const size_t nb = size_t(9) * size_t(nq + 1), nh1 = 2 * nb, nh = size_t(n_strata) * nh1;
    if (int rc = S->hist.reserve(h, nh, "stratified histogram: cannot allocate %zu bytes on the device")) return rc;
    HIPCHK(h, hipMemsetAsync(S->hist.p, 0, nh * 8, h->stream));
    int32_t *d_pb = nullptr;
    if (int rc = pr_counts_inputs(h, "vpr_pr_counts_strata", var_class, pb_phase, &d_pb)) return rc;
    const int chunk = hist_chunk(nq);
    const unsigned n_chunks = unsigned((n_strata + chunk - 1) / chunk);
    const size_t lds = size_t(std::min(chunk, n_strata)) * nb * 4;
    HIPCHK(h, hipEventRecord(S->ev[0], h->stream));
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        hipLaunchKernelGGL(k_pr_hist_strata, dim3(unsigned((nv + 255) / 256), n_chunks), dim3(256), lds, h->stream,
                           h->dB.var_off[s], h->n_sc, nv, h->d_cls[s], h->dR.sc_phase, d_pb, h->dR.v[s][0], h->dR.v[s][1],
                           s >> 1, min_qual, max_qual, words[s], n_strata, chunk, S->hist.p);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(S->ev[1], h->stream));
    std::vector<unsigned long long> hist(nh);
    if (int rc = pr_counts_finish(h, comm, S->hist.p, nh, hist.data())) return rc;
    S->ms_hist = ev_ms(S);
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(nq);
    for (int k = 0; k < n_strata; k++) pr_fold_counts(hist.data() + size_t(k) * nh1, nq, counts + size_t(k) * nc1);
    return VPR_OK;
}

}  // namespace

void strata_free(vpr_handle *h) {
    StrataState *S = h->strata;
    if (!S) return;
    release_words(h, S);
    S->hist.release(h);
    for (int k = 0; k < 2; k++) if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
    delete S;
    h->strata = nullptr;
}

// the argument checks of vpr_strata_masks: the interval tables (sorted, non-overlapping, non-empty per row) and the variant
// tables the mask kernel reads (s null: the variant tables alone)
int strata_check(vpr_handle *h, const vpr_variants *v, const vpr_strata *s) {
    if (s) {
        if (s->n_strata < 1) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: n_strata must be at least 1");
        if (s->n_ctg < 1 || s->n_ctg != v->n_ctg)
            return fail(h, VPR_ERR_ARG, "vpr_strata_masks: the strata number %d contigs, the variants %d", s->n_ctg, v->n_ctg);
    }
    if ((s && !s->iv_off) || v->n_sc < 0 || (v->n_sc > 0 && !v->sc_ctg)) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null table");
    if (s) {
        const size_t n_rows = size_t(s->n_strata) * size_t(s->n_ctg);
        if (s->iv_off[0] != 0) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: iv_off[0] is not 0");
        for (size_t r = 0; r < n_rows; r++) {
            const int64_t a = s->iv_off[r], b = s->iv_off[r + 1];
            if (b < a) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: iv_off decreases at row %zu", r);
            if (b > a && (!s->iv_start || !s->iv_stop)) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null interval table");
            if (b - a > INT32_MAX) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: more than 2^31 - 1 intervals in one row");
            const int k = int(r / size_t(s->n_ctg)), c = int(r % size_t(s->n_ctg));
            for (int64_t j = a; j < b; j++) {
                if (s->iv_stop[j] <= s->iv_start[j])
                    return fail(h, VPR_ERR_ARG, "vpr_strata_masks: stratum %d contig %d: region %d-%d has stop <= start", k, c, s->iv_start[j], s->iv_stop[j]);
                if (j > a && s->iv_start[j] < s->iv_start[j - 1])
                    return fail(h, VPR_ERR_ARG, "vpr_strata_masks: stratum %d contig %d is unsorted: region %d-%d precedes %d-%d", k, c,
                                s->iv_start[j - 1], s->iv_stop[j - 1], s->iv_start[j], s->iv_stop[j]);
                if (j > a && s->iv_start[j] < s->iv_stop[j - 1])
                    return fail(h, VPR_ERR_ARG, "vpr_strata_masks: stratum %d contig %d: regions %d-%d and %d-%d overlap", k, c,
                                s->iv_start[j - 1], s->iv_stop[j - 1], s->iv_start[j], s->iv_stop[j]);
            }
        }
    }
    const int64_t n_sc = v->n_sc;
    for (int i = 0; i < VPR_HAPS; i++) {
        if (!v->var_off[i]) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null var_off");
        if (v->var_off[i][n_sc] && (!v->var_pos[i] || !v->var_ref_len[i] || !v->var_type[i])) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null variant column");
    }
    for (int64_t k = 0; k < n_sc; k++)
        if (v->sc_ctg[k] < 0 || v->sc_ctg[k] >= v->n_ctg) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: supercluster %lld names contig %d", (long long)k, v->sc_ctg[k]);
    return VPR_OK;
}

// The membership words of the (checked) variants of `v` against interval tables that are on the device already, in the
// handle's stream order behind whatever filled them: the columns the kernel reads go up in one block that lives as long as
// the call, k_strata_mask runs once per hap slot, and the words are resident when the call returns.
int strata_masks_device(vpr_handle *h, const vpr_variants *v, int32_t n_strata, const int64_t *d_iv_off, const int32_t *d_iv_start,
                        const int32_t *d_iv_stop) {
    const int64_t n_sc = v->n_sc;
    int64_t n_var[VPR_HAPS];
    for (int i = 0; i < VPR_HAPS; i++) n_var[i] = v->var_off[i][n_sc];
    if (int rc = strata_prepare(h, n_strata, n_var)) return rc;
    StrataState *S = h->strata;
    struct Piece { const void *src; size_t bytes; size_t at; };
    std::vector<Piece> pieces;
    size_t total = 0;
    auto add = [&](const void *src, size_t bytes) { pieces.push_back({src, bytes, total}); total += (bytes + 255) & ~size_t(255); return pieces.size() - 1; };
    const size_t i_ctg = add(v->sc_ctg, 4 * size_t(n_sc));
    size_t i_var[VPR_HAPS][4];
    for (int i = 0; i < VPR_HAPS; i++) {
        i_var[i][0] = add(v->var_off[i], 8 * (size_t(n_sc) + 1));
        i_var[i][1] = add(v->var_pos[i], 4 * size_t(n_var[i]));
        i_var[i][2] = add(v->var_ref_len[i], 4 * size_t(n_var[i]));
        i_var[i][3] = add(v->var_type[i], size_t(n_var[i]));
    }
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), std::max<size_t>(total, 256), SITE) != hipSuccess) {
        (void)hipGetLastError();
        release_words(h, S);
        return fail(h, VPR_ERR_NOMEM, "vpr_strata_masks: cannot allocate %zu bytes on the device", total);
    }
    struct Release { vpr_handle *h; uint8_t *p; ~Release() { (void)hipStreamSynchronize(h->stream); (void)x_free(h, p, SITE); } } release{h, blk};
    for (const Piece &p : pieces)
        if (p.bytes && p.src) HIPCHK(h, hipMemcpyAsync(blk + p.at, p.src, p.bytes, hipMemcpyHostToDevice, h->stream));
    auto at = [&](size_t i) { return blk + pieces[i].at; };
    HIPCHK(h, hipEventRecord(S->ev[0], h->stream));
    for (int i = 0; i < VPR_HAPS; i++) {
        if (!n_var[i]) continue;
        hipLaunchKernelGGL(k_strata_mask, dim3(unsigned((n_var[i] + 255) / 256), unsigned(S->n_words)), dim3(256), 0, h->stream,
                           reinterpret_cast<const int64_t *>(at(i_var[i][0])), int(n_sc), n_var[i], reinterpret_cast<const int32_t *>(at(i_ctg)),
                           reinterpret_cast<const int32_t *>(at(i_var[i][1])), reinterpret_cast<const int32_t *>(at(i_var[i][2])), at(i_var[i][3]),
                           d_iv_off, d_iv_start, d_iv_stop, n_strata, v->n_ctg, S->words[i].p);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(S->ev[1], h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    S->ms_mask = ev_ms(S);
    S->valid = true;
    return VPR_OK;
}

// Room for n_add strata that a kernel of the caller's writes: alone (append false: as strata_prepare, *n_prev = 0) or behind the
// resident ones, whose words are kept (the word-major layout keeps the old words in front; a word array that crosses a 64-bit
// boundary is reallocated and copied).  The words are invalid until strata_commit.
int strata_extend(vpr_handle *h, const char *entry, int32_t n_add, const int64_t n_var[VPR_HAPS], bool append, int32_t *n_prev,
                  uint64_t *words[VPR_HAPS], int32_t *n_words) {
    if (!append) {
        if (int rc = strata_prepare(h, n_add, n_var)) return rc;
        *n_prev = 0;
    } else {
        StrataState *S = h->strata;
        if (!S || !S->valid)
            return fail(h, VPR_ERR_STATE, "%s: append without resident membership words (call vpr_strata_masks, vpr_context_masks or vpr_strata_upload_masks first)", entry);
        for (int s = 0; s < VPR_HAPS; s++)
            if (S->n_var[s] != n_var[s])
                return fail(h, VPR_ERR_STATE, "%s: append: the membership words hold %lld variants of hap slot %d, the variant tables %lld", entry,
                            (long long)S->n_var[s], s, (long long)n_var[s]);
        const int32_t old_words = S->n_words, new_words = (S->n_strata + n_add + 63) / 64;
        S->valid = false;
        for (int s = 0; s < VPR_HAPS; s++) {
            const size_t n = std::max<size_t>(size_t(new_words) * size_t(n_var[s]), 32);
            if (int rc = S->words[s].reserve(h, n, "stratum membership words: cannot allocate %zu bytes on the device", size_t(old_words) * size_t(n_var[s]))) {
                release_words(h, S);
                return rc;
            }
        }
        *n_prev = S->n_strata;
        S->n_strata += n_add; S->n_words = new_words;
    }
    for (int s = 0; s < VPR_HAPS; s++) words[s] = h->strata->words[s].p;
    *n_words = h->strata->n_words;
    return VPR_OK;
}

void strata_commit(vpr_handle *h) { h->strata->valid = true; }

int strata_view(vpr_handle *h, const char *entry, int32_t *n_strata, const uint64_t *words[VPR_HAPS]) {
    const StrataState *S = h->strata;
    if (!S || !S->valid)
        return fail(h, VPR_ERR_STATE, "%s: no membership words (call vpr_strata_masks or vpr_strata_upload_masks after the upload)", entry);
    for (int s = 0; s < VPR_HAPS; s++) {
        if (S->n_var[s] != h->n_var[s])
            return fail(h, VPR_ERR_STATE, "%s: the membership words hold %lld variants of hap slot %d, the executed batch has %lld", entry,
                        (long long)S->n_var[s], s, (long long)h->n_var[s]);
        words[s] = S->words[s].p;
    }
    *n_strata = S->n_strata;
    return VPR_OK;
}

extern "C" {

int vpr_strata_masks(vpr_handle *h, const vpr_variants *v, const vpr_strata *s) {
    if (!h) return VPR_ERR_ARG;
    if (!v || !s) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null argument");
    if (int rc = strata_check(h, v, s)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // ---- the interval tables: one block that lives as long as the call
    const size_t n_rows = size_t(s->n_strata) * size_t(s->n_ctg), n_iv = size_t(s->iv_off[n_rows]);
    const size_t at_st = (8 * (n_rows + 1) + 255) & ~size_t(255), at_sp = at_st + ((4 * n_iv + 255) & ~size_t(255));
    const size_t total = at_sp + ((4 * n_iv + 255) & ~size_t(255));
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), std::max<size_t>(total, 256), SITE) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, VPR_ERR_NOMEM, "vpr_strata_masks: cannot allocate %zu bytes on the device", total);
    }
    struct Release { vpr_handle *h; uint8_t *p; ~Release() { (void)hipStreamSynchronize(h->stream); (void)x_free(h, p, SITE); } } release{h, blk};
    HIPCHK(h, hipMemcpyAsync(blk, s->iv_off, 8 * (n_rows + 1), hipMemcpyHostToDevice, h->stream));
    if (n_iv) {
        HIPCHK(h, hipMemcpyAsync(blk + at_st, s->iv_start, 4 * n_iv, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(blk + at_sp, s->iv_stop, 4 * n_iv, hipMemcpyHostToDevice, h->stream));
    }
    return strata_masks_device(h, v, s->n_strata, reinterpret_cast<const int64_t *>(blk), reinterpret_cast<const int32_t *>(blk + at_st),
                               reinterpret_cast<const int32_t *>(blk + at_sp));
}

int vpr_strata_timing(const vpr_handle *h, double *ms_mask, double *ms_hist) {
    if (!h || !h->strata || !ms_mask || !ms_hist) return VPR_ERR_ARG;
    *ms_mask = h->strata->ms_mask; *ms_hist = h->strata->ms_hist;
    return VPR_OK;
}

int vpr_strata_download_masks(vpr_handle *h, uint64_t *const mask[VPR_HAPS]) {
    if (!h || !mask) return VPR_ERR_ARG;
    const StrataState *S = h->strata;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_strata_download_masks: no membership words");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (int s = 0; s < VPR_HAPS; s++) {
        const size_t bytes = size_t(S->n_words) * size_t(S->n_var[s]) * 8;
        if (!bytes) continue;
        if (!mask[s]) return fail(h, VPR_ERR_ARG, "vpr_strata_download_masks: null buffer");
        HIPCHK(h, hipMemcpyAsync(mask[s], S->words[s].p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    return VPR_OK;
}

int vpr_strata_upload_masks(vpr_handle *h, int32_t n_strata, const int64_t n_var[VPR_HAPS], const uint64_t *const mask[VPR_HAPS]) {
    if (!h) return VPR_ERR_ARG;
    if (!n_var || !mask) return fail(h, VPR_ERR_ARG, "vpr_strata_upload_masks: null argument");
    if (n_strata < 1) return fail(h, VPR_ERR_ARG, "vpr_strata_upload_masks: n_strata must be at least 1");
    for (int s = 0; s < VPR_HAPS; s++)
        if (n_var[s] < 0 || (n_var[s] && !mask[s])) return fail(h, VPR_ERR_ARG, "vpr_strata_upload_masks: bad hap slot %d", s);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = strata_prepare(h, n_strata, n_var)) return rc;
    StrataState *S = h->strata;
    for (int s = 0; s < VPR_HAPS; s++) {
        const size_t bytes = size_t(S->n_words) * size_t(n_var[s]) * 8;
        if (bytes) HIPCHK(h, hipMemcpyAsync(S->words[s].p, mask[s], bytes, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    S->valid = true;
    return VPR_OK;
}

int vpr_pr_counts_strata(vpr_handle *h, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                         int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return strata_counts_impl(h, nullptr, var_class, pb_phase, min_qual, max_qual, counts);
}

int vpr_allreduce_counts_strata(vpr_handle *h, void *nccl_comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                                int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!nccl_comm) return VPR_ERR_ARG;
    return strata_counts_impl(h, nccl_comm, var_class, pb_phase, min_qual, max_qual, counts);
}

}  // extern "C"
