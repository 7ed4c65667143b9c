// pr_labelcut.hip -- the label counts of a label pass (pr_label.h: the error classes, the match kinds) cut by stratum and resampled:
// one evaluation, one labelling, cut afterwards.  Both kernels are generic over the pass (`labels` is an argument) and read what
// is resident after the pass: its label bytes (LabelState::bytes), the membership words (pr_strata.hip), the per-variant results
// and the variant classes.  They read no variant tables and do no join.  k_label_hist_strata is k_pr_hist_strata (pr_strata.hip)
// with the label in the errtype's place; k_label_boot is its transpose, as k_pr_boot (pr_boot.hip) is of k_pr_hist_strata.  The
// bin rule is pr_counts.h's, the weight and the shape of a replicate launch pr_bootw.h's, the fold of a histogram pr_label.hip's.
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_bootw.h"
#include "pr_label.h"

namespace {

// LDS a workgroup of k_label_hist_strata may ask for: k_pr_hist_strata's budget, four workgroups beside each other in a compute unit
const size_t CUT_LDS_BUDGET = 40 * 1024;

// strata of one workgroup of k_label_hist_strata: the largest power of two up to 64 (a chunk then never straddles a membership
// word) whose privatised bins fit the budget; one stratum when even that does not (its bins then are the label call's own block
// histogram, within label_max_nq).  Seven classes at 61 thresholds: 5 208 B a stratum, 4 strata a workgroup
int cut_chunk(const LabelDesc &D, int nq) {
    const size_t per = size_t(3) * D.labels * size_t(nq + 1) * 4;
    int c = 64;
    while (c > 1 && size_t(c) * per > CUT_LDS_BUDGET) c >>= 1;
    return c;
}

}  // namespace

extern "C" {

// One lane per hap-variant, blockIdx.y a chunk of n_chunk strata (a power of two up to 64, so the chunk's bits lie in one
// membership word), whose 3 x labels x (nq + 1) bins per stratum are privatised in LDS and flushed once with 64-bit global
// atomics.  A lane with no label, or with no bit of the chunk, does nothing after its two loads.
__global__ void __launch_bounds__(256) k_label_hist_strata(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                                 const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                                 const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, const uint8_t *__restrict__ label,
                                 int labels, int callset, int min_qual, int max_qual, const uint64_t *__restrict__ words,
                                 int n_strata, int n_chunk,
                                 unsigned long long *__restrict__ hist /* [n_strata][2][3 types][labels][nq + 1] */) {
    extern __shared__ unsigned int blk[];      // [n_chunk][3][labels][nq + 1]
    const int nq = max_qual - min_qual + 1, nb = 3 * labels * (nq + 1);
    const int k0 = blockIdx.y * n_chunk, nk = min(n_chunk, n_strata - k0);
    for (int k = threadIdx.x; k < nk * nb; k += blockDim.x) blk[k] = 0;
    __syncthreads();
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n_var) {
        const int lab = label[v];
        uint64_t bits = words[size_t(k0 >> 6) * size_t(n_var) + size_t(v)] >> (k0 & 63);
        if (nk < 64) bits &= (uint64_t(1) << nk) - 1;
        if (lab < labels && bits) {
            int b = 0;
            const int row = pr_count_row(sc_of_var(var_off, n_sc, v), v, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, cls,
                                         min_qual, nq, &b);
            const int bin = ((row / 3) * labels + lab) * (nq + 1) + b;
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

// k_pr_boot over the label bins.  A workgroup owns blockIdx.y's 64 replicates, blockIdx.x's span of the slot's variants and
// blockIdx.z's slice of the quality bins (n_qs bins from blockIdx.z * n_qs; bin nq lies in exactly one slice).  Its waves take the
// span in turns, 64 variants at a time: lane = variant for the coalesced loads (label, stratum bit, supercluster, bin, key), then
// lane = replicate for the walk over those 64 by cross-lane broadcast.  The hash runs once per (lane, supercluster change); a
// variant without a label or outside the slice or the stratum is passed wave-uniformly.  span x 12 < 2^32 (BOOT_SPAN_MAX): a bin
// of the table cannot wrap.
__global__ void __launch_bounds__(1024) k_label_boot(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                          const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                          const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, const uint8_t *__restrict__ label, int labels,
                          int callset, int min_qual, int max_qual, const uint64_t *__restrict__ sc_key, uint64_t seed, int n_rep,
                          const uint64_t *__restrict__ word /* the stratum's membership word of every variant, or null */,
                          int bit, int64_t span, int n_qs,
                          unsigned long long *__restrict__ hist /* [2][3 types][labels][nq + 1][gridDim.y * 64] */) {
    extern __shared__ unsigned int tab[];      // [3 types][labels][n_qs][64]
    const int nq = max_qual - min_qual + 1, n_rows = 3 * labels, n_tab = n_rows * n_qs * 64;
    const int q_lo = blockIdx.z * n_qs;
    for (int k = threadIdx.x; k < n_tab; k += blockDim.x) tab[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int r = blockIdx.y * 64 + lane;
    const bool live = r < n_rep;
    const uint64_t salt = 0x9E3779B97F4A7C15ull * (uint64_t(r) + 1) + seed * 0xD1B54A32D192ED03ull;
    const int64_t v0 = int64_t(blockIdx.x) * span, v1 = min(n_var, v0 + span);
    int cur_sc = -1;
    uint32_t w = 0;
    for (int64_t at = v0 + int64_t(wave) * 64; at < v1; at += int64_t(n_waves) * 64) {
        // ---- lane = variant
        const int64_t v = at + lane;
        int bin = -1, sc = 0;
        uint64_t key = 0;
        if (v < v1) {
            const int lab = label[v];
            if (lab < labels && (!word || ((word[v] >> bit) & 1))) {
                sc = sc_of_var(var_off, n_sc, v);
                int b = 0;
                const int row = pr_count_row(sc, v, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, cls, min_qual, nq, &b);
                if (row >= 0 && b >= q_lo && b < q_lo + n_qs) { bin = ((row / 3) * labels + lab) * n_qs + (b - q_lo); key = sc_key[sc]; }
            }
        }
        // ---- lane = replicate
        uint64_t todo = __ballot(bin >= 0);
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int sc_j = __builtin_amdgcn_readlane(sc, j);
            if (sc_j != cur_sc) {
                cur_sc = sc_j;
                const uint32_t k_lo = __builtin_amdgcn_readlane(uint32_t(key), j), k_hi = __builtin_amdgcn_readlane(uint32_t(key >> 32), j);
                w = boot_weight((uint64_t(k_hi) << 32) | k_lo, salt);
            }
            const int bin_j = __builtin_amdgcn_readlane(bin, j);
            if (live && w) atomicAdd(&tab[bin_j * 64 + lane], w);
        }
    }
    __syncthreads();
    const size_t n_lanes = size_t(gridDim.y) * 64;
    for (int k = threadIdx.x; k < n_tab; k += blockDim.x) {
        const unsigned int c = tab[k];
        if (!c) continue;
        const int row = k >> 6, tl = row / n_qs, b = q_lo + row % n_qs;     // (b <= nq: rows beyond it are never counted into)
        atomicAdd(&hist[((size_t(callset) * n_rows + size_t(tl)) * size_t(nq + 1) + size_t(b)) * n_lanes + size_t(blockIdx.y) * 64 + size_t(k & 63)],
                  (unsigned long long)c);
    }
}

}  // extern "C"

namespace {

// What both cuts check alike, behind their own arguments: the quality range (VPR_ERR_ARG, before any allocation), the executed
// batch, valid label bytes of this pass, the classes the label call left resident
int cut_begin(vpr_handle *h, const LabelDesc &D, const char *entry, void *comm, int32_t min_qual, int32_t max_qual, LabelState **S) {
    if (max_qual < min_qual) return fail(h, VPR_ERR_ARG, "%s: max_qual %d is below min_qual %d", entry, max_qual, min_qual);
    if (int64_t(max_qual) - min_qual >= label_max_nq(D))
        return fail(h, VPR_ERR_ARG, "%s: the quality range %d..%d holds more than %d thresholds (the block histogram is in LDS)", entry, min_qual,
                    max_qual, label_max_nq(D));
    if (int rc = pr_counts_begin(h, entry, comm)) return rc;
    *S = h->label[D.pass];
    if (!*S || !(*S)->valid)
        return fail(h, VPR_ERR_STATE, "%s: no %s bytes (before %s, or after the next upload)", entry, D.noun, D.entry);
    for (int s = 0; s < VPR_HAPS; s++)
        if (h->n_var[s] && !h->d_cls[s]) return fail(h, VPR_ERR_STATE, "%s: no variant classes", entry);
    for (int k = 0; k < 2; k++) if (!(*S)->cut_ev[k]) HIPCHK(h, hipEventCreate(&(*S)->cut_ev[k]));
    return VPR_OK;
}

double cut_ms(const LabelState *S) {     // (both events have completed: the caller has synchronised the stream)
    float ms = 0;
    (void)hipEventElapsedTime(&ms, S->cut_ev[0], S->cut_ev[1]);
    return ms;
}

}  // namespace

int labelcut_strata(vpr_handle *h, const LabelDesc &D, void *comm, int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    char entry[64];
    snprintf(entry, sizeof(entry), "%s_strata", D.entry);
    if (!counts) return fail(h, VPR_ERR_ARG, "%s: null counts", entry);
    LabelState *S = nullptr;
    if (int rc = cut_begin(h, D, entry, comm, min_qual, max_qual, &S)) return rc;
    int32_t n_strata = 0;
    const uint64_t *words[VPR_HAPS];
    if (int rc = strata_view(h, entry, &n_strata, words)) return rc;
    const int nq = max_qual - min_qual + 1;
    const size_t nb = size_t(3) * D.labels * size_t(nq + 1), nh1 = 2 * nb, nh = size_t(n_strata) * nh1;
    char nomem[128];
    snprintf(nomem, sizeof(nomem), "%s: stratified %s histogram: cannot allocate %%zu bytes on the device", entry, D.noun);
    if (int rc = S->cut_hist.reserve(h, nh, nomem)) return rc;
    std::vector<unsigned long long> hist;
    try { hist.resize(nh); } catch (const std::bad_alloc &) {
        return fail(h, VPR_ERR_NOMEM, "%s: stratified %s histogram: cannot allocate %zu bytes on the host", entry, D.noun, nh * 8);
    }
    HIPCHK(h, hipMemsetAsync(S->cut_hist.p, 0, nh * 8, h->stream));
    const int chunk = cut_chunk(D, nq);
    const unsigned n_chunks = unsigned((n_strata + chunk - 1) / chunk);
    const size_t lds = size_t(std::min(chunk, n_strata)) * nb * 4;
    S->ms_strata = 0;
    S->cut_shape[0] = chunk; S->cut_shape[1] = int32_t(n_chunks); S->cut_shape[2] = int32_t(lds);
    HIPCHK(h, hipEventRecord(S->cut_ev[0], h->stream));
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        hipLaunchKernelGGL(k_label_hist_strata, dim3(unsigned((nv + 255) / 256), n_chunks), dim3(256), lds, h->stream, h->dB.var_off[s], h->n_sc,
                           nv, h->d_cls[s], h->dR.sc_phase, S->has_pb ? S->pb.p : nullptr, h->dR.v[s][0], h->dR.v[s][1], S->bytes[s].p, D.labels,
                           s >> 1, min_qual, max_qual, words[s], n_strata, chunk, S->cut_hist.p);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(S->cut_ev[1], h->stream));
    if (int rc = pr_counts_finish(h, comm, S->cut_hist.p, nh, hist.data())) return rc;
    S->ms_strata = cut_ms(S);
    const size_t nc1 = size_t(2) * VPR_VARTYPES * D.labels * size_t(nq);
    for (int k = 0; k < n_strata; k++) fold_labels(D, hist.data() + size_t(k) * nh1, nq, counts + size_t(k) * nc1);
    return VPR_OK;
}

int labelcut_boot(vpr_handle *h, const LabelDesc &D, void *comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed,
                  int32_t n_rep, int32_t stratum, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    char entry[64];
    snprintf(entry, sizeof(entry), "%s_boot", D.entry);
    if (!sc_key || !counts) return fail(h, VPR_ERR_ARG, "%s: null sc_key or counts", entry);
    if (n_rep < 1 || n_rep > VPR_BOOT_MAX_REPLICATES) return fail(h, VPR_ERR_ARG, "%s: %d replicates (1 to %d)", entry, n_rep, VPR_BOOT_MAX_REPLICATES);
    if (stratum < -1) return fail(h, VPR_ERR_ARG, "%s: stratum %d", entry, stratum);
    LabelState *S = nullptr;
    if (int rc = cut_begin(h, D, entry, comm, min_qual, max_qual, &S)) return rc;
    const uint64_t *words[VPR_HAPS] = {nullptr, nullptr, nullptr, nullptr};
    if (stratum >= 0) {
        int32_t n_strata = 0;
        if (int rc = strata_view(h, entry, &n_strata, words)) return rc;
        if (stratum >= n_strata) return fail(h, VPR_ERR_ARG, "%s: stratum %d of %d", entry, stratum, n_strata);
        for (int s = 0; s < VPR_HAPS; s++) words[s] += size_t(stratum >> 6) * size_t(h->n_var[s]);      // word-major
    }
    const int nq = max_qual - min_qual + 1, n_rows = 3 * D.labels;
    const int n_groups = (n_rep + 63) / 64;
    const size_t n_lanes = size_t(n_groups) * 64, nb = size_t(n_rows) * size_t(nq + 1), nh = 2 * nb * n_lanes;
    // the quality slices: as few as fit the LDS budget, of equal size
    const int qs_max = int(BOOT_LDS_BUDGET / (size_t(n_rows) * 64 * 4));
    const int n_slices = (nq + 1 + qs_max - 1) / qs_max, n_qs = (nq + 1 + n_slices - 1) / n_slices;
    const size_t lds = size_t(n_rows) * size_t(n_qs) * 64 * 4;
    char nomem[2][128];
    snprintf(nomem[0], sizeof(nomem[0]), "%s: replicate %s histogram: cannot allocate %%zu bytes on the device", entry, D.noun);
    snprintf(nomem[1], sizeof(nomem[1]), "%s: supercluster keys: cannot allocate %%zu bytes on the device", entry);
    if (int rc = S->cut_hist.reserve(h, nh, nomem[0])) return rc;
    if (int rc = S->keys.reserve(h, size_t(std::max(h->n_sc, 1)), nomem[1])) return rc;
    std::vector<unsigned long long> hist;
    try { hist.resize(nh); } catch (const std::bad_alloc &) {
        return fail(h, VPR_ERR_NOMEM, "%s: replicate %s histogram: cannot allocate %zu bytes on the host", entry, D.noun, nh * 8);
    }
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_label_boot), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    HIPCHK(h, hipMemsetAsync(S->cut_hist.p, 0, nh * 8, h->stream));
    if (h->n_sc) HIPCHK(h, hipMemcpyAsync(S->keys.p, sc_key, size_t(h->n_sc) * 8, hipMemcpyHostToDevice, h->stream));
    S->ms_boot = 0;
    S->cut_shape[3] = 0; S->cut_shape[4] = n_groups; S->cut_shape[5] = n_slices;
    const int n_waves = boot_waves();
    HIPCHK(h, hipEventRecord(S->cut_ev[0], h->stream));
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        const int64_t span = boot_span(nv, int64_t(n_groups) * n_slices);
        const int64_t n_spans = (nv + span - 1) / span;
        S->cut_shape[3] = std::max<int32_t>(S->cut_shape[3], int32_t(n_spans));
        hipLaunchKernelGGL(k_label_boot, dim3(unsigned(n_spans), unsigned(n_groups), unsigned(n_slices)), dim3(unsigned(n_waves) * 64), lds,
                           h->stream, h->dB.var_off[s], h->n_sc, nv, h->d_cls[s], h->dR.sc_phase, S->has_pb ? S->pb.p : nullptr, h->dR.v[s][0],
                           h->dR.v[s][1], S->bytes[s].p, D.labels, s >> 1, min_qual, max_qual, S->keys.p, seed, n_rep, words[s],
                           stratum >= 0 ? (stratum & 63) : 0, span, n_qs, S->cut_hist.p);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(S->cut_ev[1], h->stream));
    if (int rc = pr_counts_finish(h, comm, S->cut_hist.p, nh, hist.data())) return rc;
    S->ms_boot = cut_ms(S);
    // replicate r's histogram [2][3][labels][nq + 1] out of the replicate-minor device layout, then the pass's fold
    const size_t nc1 = size_t(2) * VPR_VARTYPES * D.labels * size_t(nq);
    std::vector<unsigned long long> one(2 * nb);
    for (int32_t r = 0; r < n_rep; r++) {
        for (size_t b = 0; b < 2 * nb; b++) one[b] = hist[b * n_lanes + size_t(r)];
        fold_labels(D, one.data(), nq, counts + size_t(r) * nc1);
    }
    return VPR_OK;
}

int labelcut_timing(const vpr_handle *h, const LabelDesc &D, double *ms_strata, double *ms_boot) {
    if (!h || !ms_strata || !ms_boot) return VPR_ERR_ARG;
    const LabelState *S = h->label[D.pass];
    *ms_strata = S ? S->ms_strata : 0; *ms_boot = S ? S->ms_boot : 0;
    return VPR_OK;
}

int labelcut_info(const vpr_handle *h, const LabelDesc &D, int32_t shape[6]) {
    if (!h || !shape) return VPR_ERR_ARG;
    const LabelState *S = h->label[D.pass];
    for (int k = 0; k < 6; k++) shape[k] = S ? S->cut_shape[k] : 0;
    return VPR_OK;
}
