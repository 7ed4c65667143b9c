// pr_boot.hip -- the bootstrap replicates of the precision/recall counters (include/vcfdist_bootstrap.h): the counters of
// pr_collect.hip n_rep times, with every supercluster's variants counted w(seed, replicate, key) times.
// k_pr_boot is the transpose of k_pr_hist_strata (pr_strata.hip): there a lane is a variant and the lanes of a wave pile
// onto the few bins most variants share; here a LANE IS A REPLICATE, the LDS table is [bin][64 replicates], and the 64
// increments of a wave-instruction fall on 64 consecutive words whatever the data.  The bin rule is pr_counts.h's; the weight
// and the launch shape of such a table are pr_bootw.h's (shared with k_label_boot, pr_labelcut.hip); the host
// fold of a histogram and the front and back of a counters call are the ones of pr_collect.hip.
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_bootw.h"

struct BootState {
    DevBuf<unsigned long long> hist;                             // [2][3 classes][3][nq + 1][groups * 64]: replicate-minor
    DevBuf<uint64_t> keys;                                       // the caller's sc_key
    hipEvent_t ev[2] = {nullptr, nullptr};
    int32_t grid[3] = {0, 0, 0};                                 // vpr_boot_info: spans, replicate groups, quality slices
    double ms = 0;
    bool ran = false;
};

extern "C" {

// A workgroup owns blockIdx.y's 64 replicates, blockIdx.x's span of the slot's variants and blockIdx.z's slice of the quality
// bins (n_qs bins from blockIdx.z * n_qs; bin nq, "counts at no threshold", lies in exactly one slice).  Its waves take the
// span in turns, 64 variants at a time: lane = variant for the coalesced loads (supercluster, bin, key, stratum bit), then
// lane = replicate for the walk over those 64 by cross-lane broadcast.  The hash runs once per (lane, supercluster change);
// a variant that is skipped or lies outside the slice or the stratum is passed wave-uniformly.
__global__ void __launch_bounds__(1024) k_pr_boot(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                          const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                          const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, int callset, int min_qual,
                          int max_qual, const uint64_t *__restrict__ sc_key, uint64_t seed, int n_rep,
                          const uint64_t *__restrict__ word /* the stratum's membership word of every variant, or null */,
                          int bit, int64_t span, int n_qs,
                          unsigned long long *__restrict__ hist /* [2][9][nq + 1][gridDim.y * 64] */) {
    extern __shared__ unsigned int tab[];      // [3 classes][3][n_qs][64]
    const int nq = max_qual - min_qual + 1, n_tab = 9 * n_qs * 64;
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
        if (v < v1 && (!word || ((word[v] >> bit) & 1))) {
            sc = sc_of_var(var_off, n_sc, v);
            int b = 0;
            const int row = pr_count_row(sc, v, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, cls, min_qual, nq, &b);
            if (row >= 0 && b >= q_lo && b < q_lo + n_qs) { bin = row * n_qs + (b - q_lo); key = sc_key[sc]; }
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
        const int row = k >> 6, te = row / n_qs, b = q_lo + row % n_qs;     // (b <= nq: rows beyond it are never counted into)
        atomicAdd(&hist[((size_t(callset) * 9 + size_t(te)) * size_t(nq + 1) + size_t(b)) * n_lanes + size_t(blockIdx.y) * 64 + size_t(k & 63)],
                  (unsigned long long)c);
    }
}

}  // extern "C"

namespace {

int boot_counts_impl(vpr_handle *h, void *comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase, int32_t min_qual,
                     int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep, int32_t stratum, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    if (!sc_key || !counts) return fail(h, VPR_ERR_ARG, "vpr_pr_counts_boot: null sc_key or counts");
    if (max_qual < min_qual) return fail(h, VPR_ERR_ARG, "vpr_pr_counts_boot: max_qual %d is below min_qual %d", max_qual, min_qual);
    if (n_rep < 1 || n_rep > VPR_BOOT_MAX_REPLICATES)
        return fail(h, VPR_ERR_ARG, "vpr_pr_counts_boot: %d replicates (1 to %d)", n_rep, VPR_BOOT_MAX_REPLICATES);
    if (stratum < -1) return fail(h, VPR_ERR_ARG, "vpr_pr_counts_boot: stratum %d", stratum);
    if (int rc = pr_counts_begin(h, "vpr_pr_counts_boot", comm)) return rc;
    const uint64_t *words[VPR_HAPS] = {nullptr, nullptr, nullptr, nullptr};
    if (stratum >= 0) {
        int32_t n_strata = 0;
        if (int rc = strata_view(h, "vpr_pr_counts_boot", &n_strata, words)) return rc;
        if (stratum >= n_strata) return fail(h, VPR_ERR_ARG, "vpr_pr_counts_boot: stratum %d of %d", stratum, n_strata);
        for (int s = 0; s < VPR_HAPS; s++) words[s] += size_t(stratum >> 6) * size_t(h->n_var[s]);      // word-major
    }
    if (!h->boot) h->boot = new BootState();
    BootState *S = h->boot;
    for (int k = 0; k < 2; k++) if (!S->ev[k]) HIPCHK(h, hipEventCreate(&S->ev[k]));
    const int nq = max_qual - min_qual + 1;
    const int n_groups = (n_rep + 63) / 64;
    const size_t n_lanes = size_t(n_groups) * 64, nb = size_t(9) * size_t(nq + 1), nh = 2 * nb * n_lanes;
    // the quality slices: as few as fit the LDS budget, of equal size
    const int qs_max = int(BOOT_LDS_BUDGET / (9 * 64 * 4));
    const int n_slices = (nq + 1 + qs_max - 1) / qs_max, n_qs = (nq + 1 + n_slices - 1) / n_slices;
    const size_t lds = size_t(9) * size_t(n_qs) * 64 * 4;
    if (int rc = S->hist.reserve(h, nh, "replicate histogram: cannot allocate %zu bytes on the device")) return rc;
    if (int rc = S->keys.reserve(h, size_t(std::max(h->n_sc, 1)), "supercluster keys: cannot allocate %zu bytes on the device")) return rc;
    std::vector<unsigned long long> hist;
    try { hist.resize(nh); } catch (const std::bad_alloc &) {
        return fail(h, VPR_ERR_NOMEM, "replicate histogram: cannot allocate %zu bytes on the host", nh * 8);
    }
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pr_boot), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    HIPCHK(h, hipMemsetAsync(S->hist.p, 0, nh * 8, h->stream));
    if (h->n_sc) HIPCHK(h, hipMemcpyAsync(S->keys.p, sc_key, size_t(h->n_sc) * 8, hipMemcpyHostToDevice, h->stream));
    S->grid[0] = 0; S->grid[1] = n_groups; S->grid[2] = n_slices;
    S->ms = 0; S->ran = false;
    int32_t *d_pb = nullptr;
    if (int rc = pr_counts_inputs(h, "vpr_pr_counts_boot", var_class, pb_phase, &d_pb)) return rc;
    const int n_waves = boot_waves();
    HIPCHK(h, hipEventRecord(S->ev[0], h->stream));
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        const int64_t span = boot_span(nv, int64_t(n_groups) * n_slices);
        const int64_t n_spans = (nv + span - 1) / span;
        S->grid[0] = std::max<int32_t>(S->grid[0], int32_t(n_spans));
        hipLaunchKernelGGL(k_pr_boot, dim3(unsigned(n_spans), unsigned(n_groups), unsigned(n_slices)), dim3(unsigned(n_waves) * 64), lds,
                           h->stream, h->dB.var_off[s], h->n_sc, nv, h->d_cls[s], h->dR.sc_phase, d_pb, h->dR.v[s][0], h->dR.v[s][1],
                           s >> 1, min_qual, max_qual, S->keys.p, seed, n_rep, words[s], stratum >= 0 ? (stratum & 63) : 0, span, n_qs, S->hist.p);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(S->ev[1], h->stream));
    if (int rc = pr_counts_finish(h, comm, S->hist.p, nh, hist.data())) return rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]);
    S->ms = ms; S->ran = true;
    // replicate r's histogram [2][9][nq + 1] out of the replicate-minor device layout, then the fold of vpr_pr_counts
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(nq);
    std::vector<unsigned long long> one(2 * nb);
    for (int32_t r = 0; r < n_rep; r++) {
        for (size_t b = 0; b < 2 * nb; b++) one[b] = hist[b * n_lanes + size_t(r)];
        pr_fold_counts(one.data(), nq, counts + size_t(r) * nc1);
    }
    return VPR_OK;
}

}  // namespace

void boot_free(vpr_handle *h) {
    BootState *S = h->boot;
    if (!S) return;
    dev_release(h, S->hist, S->keys);
    for (int k = 0; k < 2; k++) if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
    delete S;
    h->boot = nullptr;
}

extern "C" {

int vpr_pr_counts_boot(vpr_handle *h, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase, int32_t min_qual,
                       int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep, int32_t stratum, int64_t *counts) {
    return boot_counts_impl(h, nullptr, var_class, pb_phase, min_qual, max_qual, sc_key, seed, n_rep, stratum, counts);
}

int vpr_allreduce_counts_boot(vpr_handle *h, void *nccl_comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                              int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep,
                              int32_t stratum, int64_t *counts) {
    if (!nccl_comm) return VPR_ERR_ARG;
    return boot_counts_impl(h, nccl_comm, var_class, pb_phase, min_qual, max_qual, sc_key, seed, n_rep, stratum, counts);
}

int vpr_boot_info(const vpr_handle *h, int32_t grid[3], double *ms) {
    if (!h || !h->boot || !h->boot->ran || !grid || !ms) return VPR_ERR_ARG;
    for (int k = 0; k < 3; k++) grid[k] = h->boot->grid[k];
    *ms = h->boot->ms;
    return VPR_OK;
}

}  // extern "C"
