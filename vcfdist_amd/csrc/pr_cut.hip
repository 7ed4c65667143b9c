// pr_cut.hip -- the count cuts: the precision/recall counters (include/vcfdist_strata.h, include/vcfdist_bootstrap.h) and the
// label counts of a label pass (pr_label.h, include/vcfdist_labelcut.h), each cut by stratum and resampled.  One evaluation, one
// labelling, cut afterwards: the kernels read what is resident -- the per-variant results, the variant classes, the membership
// words (pr_strata.hip) and, for the label counts, the pass's label bytes -- and no variant tables.
// There are two device bodies, each written once over a BIN SOURCE that says how many rows a table has and which row a variant
// counts in.  hist_strata_body: a lane is a variant and counts its bin into every stratum whose bit is set.  boot_body is its
// transpose: a LANE IS A REPLICATE, the LDS table is [bin][64 replicates], and the 64 increments of a wave-instruction fall on 64
// consecutive words whatever the data.  The four kernels build their bin source and call a body; the two host drivers
// (cut_strata, cut_boot) run a cut for whoever brings a launcher and a fold.  The bin rule is pr_counts.h's; the host folds and
// the front and back of a counters call are pr_collect.hip's and pr_label.hip's.
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_cut.h"
#include "pr_label.h"
#include "../../include/vcfdist_strata.h"
#include "../../include/vcfdist_bootstrap.h"

namespace {

// ---- the bin sources (passed by value).  rows(): rows of a table.  pick(v): what the source reads of variant v ahead of
// everything else, -1 for a variant it does not count (the lane then skips the bisection and the result loads).  row(r9, p): the
// table row of a variant whose pr_count_row is r9 (class * 3 + errtype) and whose pick is p.
struct CounterBins {      // the counters: pr_count_row's own nine rows
    __device__ __forceinline__ constexpr int rows() const { return 9; }
    __device__ __forceinline__ int pick(int64_t) const { return 0; }
    __device__ __forceinline__ int row(int r9, int) const { return r9; }
};
struct LabelBins {        // the label counts: the label in the errtype's place, [3 types][labels]
    const uint8_t *__restrict__ label;
    int labels;
    __device__ __forceinline__ int rows() const { return 3 * labels; }
    __device__ __forceinline__ int pick(int64_t v) const { const int lab = label[v]; return lab < labels ? lab : -1; }
    __device__ __forceinline__ int row(int r9, int lab) const { return (r9 / 3) * labels + lab; }
};

// LDS a workgroup of a stratified histogram may ask for: four of them fit beside each other in a compute unit's 160 KiB
const size_t HIST_LDS_BUDGET = 40 * 1024;
// LDS a workgroup of a replicate table may ask for: one workgroup per compute unit (160 KiB), with room left for 64 quality bins a
// slice of the counters (9 x 64 x 64 x 4 B = 144 KiB; -mn 0 -mx 60 needs 62)
const size_t BOOT_LDS_BUDGET = 144 * 1024;
// waves of a workgroup (VPR_BOOT_WAVES: 4 .. 16).  Measured on 2 993 023 hap-variants x 1 000 replicates: 4 waves 12.3 ms,
// 8 waves 7.0 ms, 16 waves 5.2 ms (profiles/boot_bench.json): the table admits one workgroup a compute unit, so its waves
// are all the latency hiding there is
const int BOOT_WAVES = 16;
const int64_t BOOT_SPAN_MIN = 1024;               // a slot of 2 048 variants or more runs in at least two spans
const int64_t BOOT_SPAN_MAX = int64_t(1) << 24;   // x 12 < 2^32: a uint32 bin of the table cannot wrap
// workgroups of a launch from which spans stop getting shorter (VPR_BOOT_WG_TARGET).  Measured as above at 16 waves:
// 256 workgroups 4.84 ms, 512 4.86 ms, 1 024 4.95 ms, 2 048 5.18 ms, 4 096 5.93 ms, 16 384 7.50 ms -- every workgroup zeroes
// and flushes a whole table.  512 is two rounds over the 256 compute units: within 1 % of one round, less of a tail
const int64_t BOOT_WG_TARGET = 512;

__device__ const uint32_t BOOT_T[VPR_BOOT_MAX_WEIGHT] = VPR_BOOT_T;

// w(seed, r, key) of include/vcfdist_bootstrap.h: `salt` is the lane's 0x9E3779B97F4A7C15 * (r + 1) + seed * 0xD1B54A32D192ED03
__device__ inline uint32_t boot_weight(uint64_t key, uint64_t salt) {
    uint64_t z = key + salt;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const uint32_t u = uint32_t(z >> 32);
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < VPR_BOOT_MAX_WEIGHT; k++) w += u >= BOOT_T[k];
    return w;
}

// k_pr_hist (pr_collect.hip) with a stratum dimension.  One lane per hap-variant, blockIdx.y a chunk of n_chunk strata (a power of
// two up to 64, so the chunk's bits lie in one membership word), whose rows x (nq + 1) bins per stratum are privatised in LDS and
// flushed once with 64-bit global atomics.  A lane the source does not count, or with no bit of the chunk, does nothing after its
// loads.  (the columns come as four pointers: pr_counts.h)
template <typename Bins>
__device__ __forceinline__ void hist_strata_body(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var, const uint8_t *__restrict__ cls,
                                                 const int32_t *__restrict__ sc_phase, const int32_t *__restrict__ pb_phase, const uint8_t *e0,
                                                 const uint8_t *e1, const float *q0, const float *q1, const Bins src, int callset, int min_qual,
                                                 int max_qual, const uint64_t *__restrict__ words, int n_strata, int n_chunk,
                                                 unsigned long long *__restrict__ hist /* [n_strata][2][rows][nq + 1] */) {
    extern __shared__ unsigned int blk[];      // [n_chunk][rows][nq + 1]
    const unsigned nt = blockDim.x;            // (read once: behind the barrier the inlined body otherwise fetches it with vector loads)
    const int nq = max_qual - min_qual + 1, nb = src.rows() * (nq + 1);
    const int k0 = blockIdx.y * n_chunk, nk = min(n_chunk, n_strata - k0);
    for (int k = threadIdx.x; k < nk * nb; k += nt) blk[k] = 0;
    __syncthreads();
    const int64_t v = int64_t(blockIdx.x) * nt + threadIdx.x;
    if (v < n_var) {
        const int p = src.pick(v);
        uint64_t bits = words[size_t(k0 >> 6) * size_t(n_var) + size_t(v)] >> (k0 & 63);
        if (nk < 64) bits &= (uint64_t(1) << nk) - 1;
        if (p >= 0 && bits) {
            int b = 0;
            const int row = pr_count_row(sc_of_var(var_off, n_sc, v), v, sc_phase, pb_phase, e0, e1, q0, q1, cls, min_qual, nq, &b);
            const int bin = src.row(row, p) * (nq + 1) + b;
            while (row >= 0 && bits) {
                const int j = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                atomicAdd(&blk[j * nb + bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nk * nb; k += nt)
        if (blk[k]) atomicAdd(&hist[(size_t(k0 + k / nb) * 2 + size_t(callset)) * nb + size_t(k % nb)], (unsigned long long)blk[k]);
}

// A workgroup owns blockIdx.y's 64 replicates, blockIdx.x's span of the slot's variants and blockIdx.z's slice of the quality
// bins (n_qs bins from blockIdx.z * n_qs; bin nq, "counts at no threshold", lies in exactly one slice).  Its waves take the
// span in turns, 64 variants at a time: lane = variant for the coalesced loads (the source's pick, stratum bit, supercluster, bin,
// key), then lane = replicate for the walk over those 64 by cross-lane broadcast.  The hash runs once per (lane, supercluster
// change); a variant that is not counted or lies outside the slice or the stratum is passed wave-uniformly.
template <typename Bins>
__device__ __forceinline__ void boot_body(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var, const uint8_t *__restrict__ cls,
                                          const int32_t *__restrict__ sc_phase, const int32_t *__restrict__ pb_phase, const uint8_t *e0,
                                          const uint8_t *e1, const float *q0, const float *q1, const Bins src, int callset, int min_qual,
                                          int max_qual, const uint64_t *__restrict__ sc_key, uint64_t seed, int n_rep,
                                          const uint64_t *__restrict__ word /* the stratum's membership word of every variant, or null */,
                                          int bit, int64_t span, int n_qs,
                                          unsigned long long *__restrict__ hist /* [2][rows][nq + 1][gridDim.y * 64] */) {
    extern __shared__ unsigned int tab[];      // [rows][n_qs][64]
    const unsigned nt = blockDim.x;            // (read once, as in hist_strata_body)
    const int nq = max_qual - min_qual + 1, n_rows = src.rows(), n_tab = n_rows * n_qs * 64;
    const int q_lo = blockIdx.z * n_qs;
    for (int k = threadIdx.x; k < n_tab; k += nt) tab[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = nt >> 6;
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
            const int p = src.pick(v);
            if (p >= 0 && (!word || ((word[v] >> bit) & 1))) {
                sc = sc_of_var(var_off, n_sc, v);
                int b = 0;
                const int row = pr_count_row(sc, v, sc_phase, pb_phase, e0, e1, q0, q1, cls, min_qual, nq, &b);
                if (row >= 0 && b >= q_lo && b < q_lo + n_qs) { bin = src.row(row, p) * n_qs + (b - q_lo); key = sc_key[sc]; }
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
    for (int k = threadIdx.x; k < n_tab; k += nt) {
        const unsigned int c = tab[k];
        if (!c) continue;
        const int row = k >> 6, tr = row / n_qs, b = q_lo + row % n_qs;     // (b <= nq: rows beyond it are never counted into)
        atomicAdd(&hist[((size_t(callset) * n_rows + size_t(tr)) * size_t(nq + 1) + size_t(b)) * n_lanes + size_t(blockIdx.y) * 64 + size_t(k & 63)],
                  (unsigned long long)c);
    }
}

}  // namespace

extern "C" {

__global__ void __launch_bounds__(256) k_pr_hist_strata(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                                 const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                                 const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, int callset, int min_qual,
                                 int max_qual, const uint64_t *__restrict__ words, int n_strata, int n_chunk,
                                 unsigned long long *__restrict__ hist /* [n_strata][2][3 classes][3][nq + 1] */) {
    hist_strata_body(var_off, n_sc, n_var, cls, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, CounterBins{}, callset, min_qual,
                     max_qual, words, n_strata, n_chunk, hist);
}

__global__ void __launch_bounds__(256) k_label_hist_strata(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                                 const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                                 const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, const uint8_t *__restrict__ label,
                                 int labels, int callset, int min_qual, int max_qual, const uint64_t *__restrict__ words,
                                 int n_strata, int n_chunk,
                                 unsigned long long *__restrict__ hist /* [n_strata][2][3 types][labels][nq + 1] */) {
    hist_strata_body(var_off, n_sc, n_var, cls, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, LabelBins{label, labels}, callset,
                     min_qual, max_qual, words, n_strata, n_chunk, hist);
}

__global__ void __launch_bounds__(1024) k_pr_boot(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                          const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                          const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, int callset, int min_qual,
                          int max_qual, const uint64_t *__restrict__ sc_key, uint64_t seed, int n_rep,
                          const uint64_t *__restrict__ word, int bit, int64_t span, int n_qs,
                          unsigned long long *__restrict__ hist /* [2][3 classes][3][nq + 1][gridDim.y * 64] */) {
    boot_body(var_off, n_sc, n_var, cls, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, CounterBins{}, callset, min_qual,
              max_qual, sc_key, seed, n_rep, word, bit, span, n_qs, hist);
}

// (span x 12 < 2^32, BOOT_SPAN_MAX: a bin of either table cannot wrap)
__global__ void __launch_bounds__(1024) k_label_boot(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                          const uint8_t *__restrict__ cls, const int32_t *__restrict__ sc_phase,
                          const int32_t *__restrict__ pb_phase, VarCols c0, VarCols c1, const uint8_t *__restrict__ label, int labels,
                          int callset, int min_qual, int max_qual, const uint64_t *__restrict__ sc_key, uint64_t seed, int n_rep,
                          const uint64_t *__restrict__ word, int bit, int64_t span, int n_qs,
                          unsigned long long *__restrict__ hist /* [2][3 types][labels][nq + 1][gridDim.y * 64] */) {
    boot_body(var_off, n_sc, n_var, cls, sc_phase, pb_phase, c0.errtype, c1.errtype, c0.callq, c1.callq, LabelBins{label, labels}, callset,
              min_qual, max_qual, sc_key, seed, n_rep, word, bit, span, n_qs, hist);
}

}  // extern "C"

// ---- the state (pr_cut.h)
int cut_mark(vpr_handle *h, CutState &C, int k) {
    if (!C.ev[k]) HIPCHK(h, hipEventCreate(&C.ev[k]));
    HIPCHK(h, hipEventRecord(C.ev[k], h->stream));
    return VPR_OK;
}

double cut_elapsed(const CutState &C) {     // (both events have completed: the caller has synchronised the stream)
    float ms = 0;
    (void)hipEventElapsedTime(&ms, C.ev[0], C.ev[1]);
    return ms;
}

void cut_release(vpr_handle *h, CutState &C) {
    dev_release(h, C.hist, C.keys);
    for (hipEvent_t &e : C.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

namespace {

// the first arguments of all four kernels: hap slot s of the executed batch under the phase-block phasing pb
#define CUT_SLOT_ARGS(h, s, pb) (h)->dB.var_off[s], (h)->n_sc, (h)->n_var[s], (h)->d_cls[s], (h)->dR.sc_phase, pb, (h)->dR.v[s][0], (h)->dR.v[s][1]

// room for the nh words of a cut's histogram on the device (zeroed, in stream order) and on the host
int cut_room(vpr_handle *h, const char *entry, const char *what, CutState &C, size_t nh, std::vector<unsigned long long> &hist) {
    char nomem[128];
    snprintf(nomem, sizeof(nomem), "%s: %s histogram: cannot allocate %%zu bytes on the device", entry, what);
    if (int rc = C.hist.reserve(h, nh, nomem)) return rc;
    try { hist.resize(nh); } catch (const std::bad_alloc &) {
        return fail(h, VPR_ERR_NOMEM, "%s: %s histogram: cannot allocate %zu bytes on the host", entry, what, nh * 8);
    }
    HIPCHK(h, hipMemsetAsync(C.hist.p, 0, nh * 8, h->stream));
    return VPR_OK;
}

// A stratified count of `rows`-row tables over the n_strata resident strata.  inputs() puts what the entry's kernel reads besides
// the resident state on the device (behind the cleared histogram, in front of the timed launches); launch(s, grid, lds, chunk)
// enqueues the kernel of hap slot s on h->stream, 256 threads a workgroup, into C.hist; fold(hist, k) turns stratum k's histogram
// [2][rows][nq + 1] into the caller's counts.  comm non-null: one all-reduce of the histograms in between.
template <typename Inputs, typename Launch, typename Fold>
int cut_strata(vpr_handle *h, const char *entry, void *comm, CutState &C, int32_t min_qual, int32_t max_qual, int rows, int32_t n_strata,
               Inputs inputs, Launch launch, Fold fold) {
    const int nq = max_qual - min_qual + 1;
    const size_t nb = size_t(rows) * size_t(nq + 1), nh1 = 2 * nb, nh = size_t(n_strata) * nh1;
    std::vector<unsigned long long> hist;
    if (int rc = cut_room(h, entry, "stratified", C, nh, hist)) return rc;
    if (int rc = inputs()) return rc;
    // strata of one workgroup: the largest power of two up to 64 (a chunk then never straddles a membership word) whose privatised
    // bins fit the budget; one stratum when even that does not (the label counts' bins then are the label call's own block
    // histogram, within label_max_nq).  The counters at 61 thresholds: 2 232 B a stratum, 16 strata a workgroup; seven classes: 5 208 B, 4
    int chunk = 64;
    while (chunk > 1 && size_t(chunk) * nb * 4 > HIST_LDS_BUDGET) chunk >>= 1;
    const unsigned n_chunks = unsigned((n_strata + chunk - 1) / chunk);
    const size_t lds = size_t(std::min(chunk, n_strata)) * nb * 4;
    C.ms_strata = 0;
    C.shape[0] = C.shape[1] = C.shape[2] = 0;
    if (int rc = cut_mark(h, C, 0)) return rc;
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        launch(s, dim3(unsigned((nv + 255) / 256), n_chunks), lds, chunk);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = cut_mark(h, C, 1)) return rc;
    if (int rc = pr_counts_finish(h, comm, C.hist.p, nh, hist.data())) return rc;
    C.ms_strata = cut_elapsed(C);
    C.shape[0] = chunk; C.shape[1] = int32_t(n_chunks); C.shape[2] = int32_t(lds);
    for (int k = 0; k < n_strata; k++) fold(hist.data() + size_t(k) * nh1, size_t(k));
    return VPR_OK;
}

// the arguments every replicate entry checks alike, behind its null checks
int boot_check(vpr_handle *h, const char *entry, int32_t n_rep, int32_t stratum) {
    if (n_rep < 1 || n_rep > VPR_BOOT_MAX_REPLICATES) return fail(h, VPR_ERR_ARG, "%s: %d replicates (1 to %d)", entry, n_rep, VPR_BOOT_MAX_REPLICATES);
    if (stratum < -1) return fail(h, VPR_ERR_ARG, "%s: stratum %d", entry, stratum);
    return VPR_OK;
}

// word[s]: the membership word that holds `stratum`'s bit, of every variant of hap slot s; null for stratum -1 (no mask)
int boot_words(vpr_handle *h, const char *entry, int32_t stratum, const uint64_t *word[VPR_HAPS]) {
    for (int s = 0; s < VPR_HAPS; s++) word[s] = nullptr;
    if (stratum < 0) return VPR_OK;
    int32_t n_strata = 0;
    if (int rc = strata_view(h, entry, &n_strata, word)) return rc;
    if (stratum >= n_strata) return fail(h, VPR_ERR_ARG, "%s: stratum %d of %d", entry, stratum, n_strata);
    for (int s = 0; s < VPR_HAPS; s++) word[s] += size_t(stratum >> 6) * size_t(h->n_var[s]);      // word-major
    return VPR_OK;
}

int boot_waves() {
    int n = BOOT_WAVES;
    if (const char *e = getenv("VPR_BOOT_WAVES")) n = atoi(e);      // diagnostic
    return std::max(4, std::min(16, n));
}

// variants of a span of a slot of nv variants, in a launch whose other grid dimensions multiply to `others`
int64_t boot_span(int64_t nv, int64_t others) {
    int64_t target = BOOT_WG_TARGET;
    if (const char *e = getenv("VPR_BOOT_WG_TARGET")) target = std::max(1, atoi(e));      // diagnostic
    const int64_t want = std::max<int64_t>(2, (target + others - 1) / others);
    int64_t span = std::max(BOOT_SPAN_MIN, (nv + want - 1) / want);
    span = (span + 63) & ~int64_t(63);
    return std::min(span, BOOT_SPAN_MAX);
}

// A replicate count of `rows`-row tables: n_rep replicates under the caller's sc_key.  inputs() as for cut_strata;
// launch(s, grid, block, lds, span, n_qs) enqueues `kernel` for hap slot s on h->stream, with C.keys and into C.hist; fold(hist, r)
// turns replicate r's histogram [2][rows][nq + 1] into the caller's counts.  comm non-null: one all-reduce in between.
template <typename Inputs, typename Launch, typename Fold>
int cut_boot(vpr_handle *h, const char *entry, void *comm, CutState &C, int32_t min_qual, int32_t max_qual, int rows, const void *kernel,
             const uint64_t *sc_key, int32_t n_rep, Inputs inputs, Launch launch, Fold fold) {
    const int nq = max_qual - min_qual + 1;
    const int n_groups = (n_rep + 63) / 64;
    const size_t n_lanes = size_t(n_groups) * 64, nb = size_t(rows) * size_t(nq + 1), nh = 2 * nb * n_lanes;
    // the quality slices: as few as fit the LDS budget, of equal size
    const int qs_max = int(BOOT_LDS_BUDGET / (size_t(rows) * 64 * 4));
    const int n_slices = (nq + 1 + qs_max - 1) / qs_max, n_qs = (nq + 1 + n_slices - 1) / n_slices;
    const size_t lds = size_t(rows) * size_t(n_qs) * 64 * 4;
    char nomem[128];
    snprintf(nomem, sizeof(nomem), "%s: supercluster keys: cannot allocate %%zu bytes on the device", entry);
    if (int rc = C.keys.reserve(h, size_t(std::max(h->n_sc, 1)), nomem)) return rc;
    std::vector<unsigned long long> hist;
    if (int rc = cut_room(h, entry, "replicate", C, nh, hist)) return rc;
    HIPCHK(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    if (h->n_sc) HIPCHK(h, hipMemcpyAsync(C.keys.p, sc_key, size_t(h->n_sc) * 8, hipMemcpyHostToDevice, h->stream));
    if (int rc = inputs()) return rc;
    C.ms_boot = 0;
    C.shape[3] = C.shape[4] = C.shape[5] = 0;
    const int n_waves = boot_waves();
    int32_t max_spans = 0;
    if (int rc = cut_mark(h, C, 0)) return rc;
    for (int s = 0; s < VPR_HAPS; s++) {
        const int64_t nv = h->n_var[s];
        if (!nv) continue;
        const int64_t span = boot_span(nv, int64_t(n_groups) * n_slices);
        const int64_t n_spans = (nv + span - 1) / span;
        max_spans = std::max(max_spans, int32_t(n_spans));
        launch(s, dim3(unsigned(n_spans), unsigned(n_groups), unsigned(n_slices)), dim3(unsigned(n_waves) * 64), lds, span, n_qs);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = cut_mark(h, C, 1)) return rc;
    if (int rc = pr_counts_finish(h, comm, C.hist.p, nh, hist.data())) return rc;
    C.ms_boot = cut_elapsed(C);
    C.shape[3] = max_spans; C.shape[4] = n_groups; C.shape[5] = n_slices;
    // replicate r's histogram out of the replicate-minor device layout, then the caller's fold
    std::vector<unsigned long long> one(2 * nb);
    for (int32_t r = 0; r < n_rep; r++) {
        for (size_t b = 0; b < 2 * nb; b++) one[b] = hist[b * n_lanes + size_t(r)];
        fold(one.data(), size_t(r));
    }
    return VPR_OK;
}

// ---- the counters (include/vcfdist_strata.h, include/vcfdist_bootstrap.h)
int strata_counts_impl(vpr_handle *h, void *comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                       int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!h || !counts || max_qual < min_qual) return VPR_ERR_ARG;
    const char *entry = "vpr_pr_counts_strata";
    if (int rc = pr_counts_begin(h, entry, comm)) return rc;
    int32_t n_strata = 0;
    const uint64_t *words[VPR_HAPS];
    if (int rc = strata_view(h, entry, &n_strata, words)) return rc;
    int32_t *d_pb = nullptr;
    CutState &C = strata_cut(h);
    const int nq = max_qual - min_qual + 1;
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(nq);
    return cut_strata(h, entry, comm, C, min_qual, max_qual, 9, n_strata,
        [&] { return pr_counts_inputs(h, entry, var_class, pb_phase, &d_pb); },
        [&](int s, dim3 grid, size_t lds, int chunk) {
            hipLaunchKernelGGL(k_pr_hist_strata, grid, dim3(256), lds, h->stream, CUT_SLOT_ARGS(h, s, d_pb), s >> 1, min_qual, max_qual, words[s],
                               n_strata, chunk, C.hist.p);
        },
        [&](const unsigned long long *hist, size_t k) { pr_fold_counts(hist, nq, counts + k * nc1); });
}

int boot_counts_impl(vpr_handle *h, void *comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase, int32_t min_qual,
                     int32_t max_qual, const uint64_t *sc_key, uint64_t seed, int32_t n_rep, int32_t stratum, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    const char *entry = "vpr_pr_counts_boot";
    if (!sc_key || !counts) return fail(h, VPR_ERR_ARG, "%s: null sc_key or counts", entry);
    if (max_qual < min_qual) return fail(h, VPR_ERR_ARG, "%s: max_qual %d is below min_qual %d", entry, max_qual, min_qual);
    if (int rc = boot_check(h, entry, n_rep, stratum)) return rc;
    if (int rc = pr_counts_begin(h, entry, comm)) return rc;
    const uint64_t *word[VPR_HAPS];
    if (int rc = boot_words(h, entry, stratum, word)) return rc;
    if (!h->boot) h->boot = new CutState();
    CutState &C = *h->boot;
    int32_t *d_pb = nullptr;
    const int nq = max_qual - min_qual + 1, bit = stratum >= 0 ? (stratum & 63) : 0;
    const size_t nc1 = size_t(2) * VPR_VARTYPES * 3 * size_t(nq);
    return cut_boot(h, entry, comm, C, min_qual, max_qual, 9, reinterpret_cast<const void *>(k_pr_boot), sc_key, n_rep,
        [&] { return pr_counts_inputs(h, entry, var_class, pb_phase, &d_pb); },
        [&](int s, dim3 grid, dim3 block, size_t lds, int64_t span, int n_qs) {
            hipLaunchKernelGGL(k_pr_boot, grid, block, lds, h->stream, CUT_SLOT_ARGS(h, s, d_pb), s >> 1, min_qual, max_qual, C.keys.p, seed, n_rep,
                               word[s], bit, span, n_qs, C.hist.p);
        },
        [&](const unsigned long long *hist, size_t r) { pr_fold_counts(hist, nq, counts + r * nc1); });
}

// ---- the label counts (pr_label.h).  What both cuts check alike, behind their own arguments: the quality range (VPR_ERR_ARG,
// before any allocation), the executed batch, valid label bytes of this pass, the classes the label call left resident
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
    return VPR_OK;
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
    const int32_t *d_pb = S->has_pb ? S->pb.p : nullptr;      // the phasing the bytes were made under
    const int nq = max_qual - min_qual + 1;
    const size_t nc1 = size_t(2) * VPR_VARTYPES * D.labels * size_t(nq);
    return cut_strata(h, entry, comm, S->cut, min_qual, max_qual, 3 * D.labels, n_strata, [] { return VPR_OK; },
        [&](int s, dim3 grid, size_t lds, int chunk) {
            hipLaunchKernelGGL(k_label_hist_strata, grid, dim3(256), lds, h->stream, CUT_SLOT_ARGS(h, s, d_pb), S->bytes[s].p, D.labels, s >> 1,
                               min_qual, max_qual, words[s], n_strata, chunk, S->cut.hist.p);
        },
        [&](const unsigned long long *hist, size_t k) { fold_labels(D, hist, nq, counts + k * nc1); });
}

int labelcut_boot(vpr_handle *h, const LabelDesc &D, void *comm, int32_t min_qual, int32_t max_qual, const uint64_t *sc_key, uint64_t seed,
                  int32_t n_rep, int32_t stratum, int64_t *counts) {
    if (!h) return VPR_ERR_ARG;
    char entry[64];
    snprintf(entry, sizeof(entry), "%s_boot", D.entry);
    if (!sc_key || !counts) return fail(h, VPR_ERR_ARG, "%s: null sc_key or counts", entry);
    if (int rc = boot_check(h, entry, n_rep, stratum)) return rc;
    LabelState *S = nullptr;
    if (int rc = cut_begin(h, D, entry, comm, min_qual, max_qual, &S)) return rc;
    const uint64_t *word[VPR_HAPS];
    if (int rc = boot_words(h, entry, stratum, word)) return rc;
    const int32_t *d_pb = S->has_pb ? S->pb.p : nullptr;      // the phasing the bytes were made under
    const int nq = max_qual - min_qual + 1, bit = stratum >= 0 ? (stratum & 63) : 0;
    const size_t nc1 = size_t(2) * VPR_VARTYPES * D.labels * size_t(nq);
    return cut_boot(h, entry, comm, S->cut, min_qual, max_qual, 3 * D.labels, reinterpret_cast<const void *>(k_label_boot), sc_key, n_rep,
        [] { return VPR_OK; },
        [&](int s, dim3 grid, dim3 block, size_t lds, int64_t span, int n_qs) {
            hipLaunchKernelGGL(k_label_boot, grid, block, lds, h->stream, CUT_SLOT_ARGS(h, s, d_pb), S->bytes[s].p, D.labels, s >> 1, min_qual,
                               max_qual, S->cut.keys.p, seed, n_rep, word[s], bit, span, n_qs, S->cut.hist.p);
        },
        [&](const unsigned long long *hist, size_t r) { fold_labels(D, hist, nq, counts + r * nc1); });
}

int labelcut_timing(const vpr_handle *h, const LabelDesc &D, double *ms_strata, double *ms_boot) {
    if (!h || !ms_strata || !ms_boot) return VPR_ERR_ARG;
    const LabelState *S = h->label[D.pass];
    *ms_strata = S ? S->cut.ms_strata : 0; *ms_boot = S ? S->cut.ms_boot : 0;
    return VPR_OK;
}

int labelcut_info(const vpr_handle *h, const LabelDesc &D, int32_t shape[6]) {
    if (!h || !shape) return VPR_ERR_ARG;
    const LabelState *S = h->label[D.pass];
    for (int k = 0; k < 6; k++) shape[k] = S ? S->cut.shape[k] : 0;
    return VPR_OK;
}

void boot_free(vpr_handle *h) {
    if (!h->boot) return;
    cut_release(h, *h->boot);
    delete h->boot;
    h->boot = nullptr;
}

extern "C" {

int vpr_pr_counts_strata(vpr_handle *h, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                         int32_t min_qual, int32_t max_qual, int64_t *counts) {
    return strata_counts_impl(h, nullptr, var_class, pb_phase, min_qual, max_qual, counts);
}

int vpr_allreduce_counts_strata(vpr_handle *h, void *nccl_comm, const uint8_t *const var_class[VPR_HAPS], const int32_t *pb_phase,
                                int32_t min_qual, int32_t max_qual, int64_t *counts) {
    if (!nccl_comm) return VPR_ERR_ARG;
    return strata_counts_impl(h, nccl_comm, var_class, pb_phase, min_qual, max_qual, counts);
}

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

// (shape[4], the replicate groups, is nonzero exactly after a call that succeeded)
int vpr_boot_info(const vpr_handle *h, int32_t grid[3], double *ms) {
    if (!h || !h->boot || !h->boot->shape[4] || !grid || !ms) return VPR_ERR_ARG;
    for (int k = 0; k < 3; k++) grid[k] = h->boot->shape[3 + k];
    *ms = h->boot->ms_boot;
    return VPR_OK;
}

}  // extern "C"
