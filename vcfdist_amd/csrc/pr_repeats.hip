// pr_repeats.hip -- the repeat strata (include/vcfdist_repeats.h): sorted interval lists per (stratum, contig) of the bases covered
// by a k-mer that occurs more than once in the genome, on either strand.
//
// Unlike the predicates of pr_context.hip this one is not local: every k-mer is compared with every other, across contigs.  The
// genome-wide part is therefore a step of its own, in front of pr_context.hip's run passes.  Per stratum (k, slop):
//   1. k_rep_pack<false>, a scan, k_rep_pack<true>   a lane takes 16 consecutive starts (its 16 bytes and a halo of k - 1 <= 31, three
//                                                    16-byte loads), rolls fwd and rc two bits per base and keeps a count of called
//                                                    bases since the last uncalled one or contig start, so validity costs no rescan;
//                                                    (canon, global start) of the valid starts are written at prefix sums of the
//                                                    workgroups' counts (through LDS, so that the stores are coalesced) -- no
//                                                    atomic cursor, two calls give identical arrays
//   2. vplan_sort_pairs_u64 (pr_plan.hip)            rocPRIM's radix sort over key bits [0, 2k), genome-wide, not split
//   3. k_rep_mark                                    sorted element j is repeated iff its key equals a neighbour's; its bit is set
//                                                    (a return-less atomicOr on 32-bit words: OR commutes, the words come out the
//                                                    same whatever the order) at the k-mer's LAST base, global position start + k - 1
//   4. k_rep_piece_words, ctx_intervals_from_flags   per piece of whole contigs: with the flag at the last base, a run [a + k - 1,
//                                                    b + k - 1) of flags under the period rule "tract = [run start - p, run end)",
//                                                    p = k - 1, is the tract [a, b - 1 + k) of the header; min_len 1, no primitive
//                                                    test (that is a rule of the period strata); pad, merge and rows as there
//
// The host side of these steps is KmerWork (pr_kmer.h, defined at the end of this file beside the kernels it launches), which
// pr_longrepeats.hip uses too; the rows end in a KmerState.  Device memory: the formula of pr_kmer.h, the pairs being the valid
// starts of the entry with the most.  The buckets KmerState::ms[0..3] are pack, sort, mark, intervals.
#include "pr_kmer.h"
#include "pr_plan.h"
#include "pr_ctxdev.h"

namespace {

const int REP_LANE = 16, REP_WG = 256, REP_TILE = REP_LANE * REP_WG;      // the pack kernels: starts of a lane / a workgroup
const int REP_HALO = VPR_REP_MAX_K - 1;                                    // bases behind a lane's 16 that its last start reads
const unsigned MARK_MAX_WG = 4096;                                         // workgroups of the mark kernel (k_rep_mark)
const int REP_WORDS = (REP_LANE + REP_HALO + 15) / 16 * 4;                 // the lane's bytes as 32-bit words: three 16-byte loads

const vpr_repeat_stratum DEFAULT_SPEC[] = {{16, 0}, {24, 0}, {32, 0}};
const char *const DEFAULT_NAMES[] = {"rep_k16", "rep_k24", "rep_k32"};
const char *const ENTRY = "vpr_repeat_intervals";

// The starts G .. G + 15 of one lane, whose bytes [G, G + 48) are in w: returns how many are valid and, with EMIT, writes their
// (canon, start) -- with FWD (fwd, start), the forward code, for a caller that tells the strands apart (pr_nearrepeats.hip) -- from
// keys[at] / vals[at] on in start order.  Base G + jj is consumed at step jj; the k-mer that ends there starts
// at G + jj - (k - 1) and is valid iff the last k bases consumed were called and no contig began behind the first of them.
template <bool EMIT, bool FWD = false>
__device__ inline uint32_t rep_roll(const uint32_t (&w)[REP_WORDS], int64_t G, const int64_t *__restrict__ ctg_off, int n_ctg, int k,
                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t at) {
    int c = ctg_of(ctg_off, n_ctg, G);
    int64_t ce = ctg_off[c + 1];
    const uint64_t mask = k == 32 ? ~uint64_t(0) : (uint64_t(1) << (2 * k)) - 1;
    const int top = 2 * (k - 1);
    uint64_t fwd = 0, rc = 0;
    int run = 0;                         // called bases since the last uncalled base or contig start, up to and with this one
    uint32_t n = 0;
#pragma unroll
    for (int jj = 0; jj < REP_LANE + REP_HALO; jj++) {
        if (jj >= REP_LANE - 1 + k) continue;                                 // (uniform: k is the launch's)
        const int64_t Gp = G + jj;
        if (Gp >= ce) {                  // a contig begins at or before this base (or the genome has ended: zero bytes, not called)
            run = 0;
            while (Gp >= ce && c + 1 < n_ctg) { c++; ce = ctg_off[c + 1]; }
        }
        const unsigned x = (w[jj >> 2] >> ((jj & 3) * 8)) & 255u;
        const unsigned code = ((x >> 1) ^ (x >> 2)) & 3u;                     // A 0, C 1, G 2, T 3
        run = called(x) ? run + 1 : 0;
        if (EMIT) {
            fwd = ((fwd << 2) | code) & mask;
            rc = (rc >> 2) | (uint64_t(3u - code) << top);
        }
        if (jj >= k - 1 && run >= k) {
            if (EMIT) { keys[at + n] = FWD || fwd < rc ? fwd : rc; vals[at + n] = uint32_t(Gp - (k - 1)); }
            n++;
        }
    }
    return n;
}

}  // namespace

// WRITE false: the workgroup's count of valid starts into out[blockIdx.x].  WRITE true: out holds the exclusive scan of those
// counts; every lane puts its valid starts behind those of the lanes before it into LDS, and the workgroup copies the tile's
// pairs out behind its offset with consecutive lanes on consecutive elements (a lane storing its own 16 directly would put the
// 64 lanes of a store on 64 different lines).
template <bool WRITE, bool FWD>
__global__ void __launch_bounds__(256) k_rep_pack(const uint8_t *__restrict__ seq, const int64_t *__restrict__ ctg_off, int n_ctg, int64_t N, int k,
                                                  uint32_t *__restrict__ out, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    __shared__ uint32_t lds[4];
    const int64_t G = (int64_t(blockIdx.x) * REP_WG + threadIdx.x) * REP_LANE;
    uint32_t w[REP_WORDS];
    uint32_t n = 0;
    const bool live = G < N;             // (the sequence is padded with zero bytes so that the three loads of a live lane stay inside)
    if (live) {
#pragma unroll
        for (int q = 0; q < REP_WORDS / 4; q++) {
            const uint4 v = *reinterpret_cast<const uint4 *>(seq + G + 16 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        n = rep_roll<false>(w, G, ctg_off, n_ctg, k, nullptr, nullptr, 0u);
    }
    uint32_t total;
    const uint32_t before = block_scan(n, lds, &total);
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) out[blockIdx.x] = total;
    } else {
        __shared__ uint64_t tile_keys[REP_TILE];
        __shared__ uint32_t tile_vals[REP_TILE];
        if (n) (void)rep_roll<true, FWD>(w, G, ctg_off, n_ctg, k, tile_keys, tile_vals, before);      // (before + n <= total <= REP_TILE)
        __syncthreads();
        const uint32_t at = out[blockIdx.x];
        for (uint32_t i = threadIdx.x; i < total; i += REP_WG) { keys[at + i] = tile_keys[i]; vals[at + i] = tile_vals[i]; }
    }
}

extern "C" {

// element j of the sorted pairs is a repeated start iff a neighbour has its key; flag bit start + k - 1, and the count.  A grid of at
// most MARK_MAX_WG workgroups strides over the elements: the one add per workgroup goes to ONE address, and as many adds as a
// workgroup per 256 elements would make took longer than the pass itself.
__global__ void __launch_bounds__(256) k_rep_mark(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n, int k,
                                                  uint32_t *__restrict__ flags32, unsigned long long *__restrict__ n_rep) {
    __shared__ uint32_t lds[4];
    uint32_t mine = 0;                   // (at most n / 256 / gridDim.x + 1 <= 2^32 / 256 / MARK_MAX_WG + 1 a lane)
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < n; j += uint64_t(gridDim.x) * 256) {
        const uint64_t key = keys[j];
        if ((j > 0 && keys[j - 1] == key) || (j + 1 < n && keys[j + 1] == key)) {
            const uint64_t pos = uint64_t(vals[j]) + uint64_t(k - 1);
            atomicOr(&flags32[pos >> 5], 1u << (pos & 31));
            mine++;
        }
    }
    uint32_t total;
    (void)block_scan(mine, lds, &total);
    if (threadIdx.x == 0 && total) atomicAdd(n_rep, (unsigned long long)total);
}

// the flag words of a piece: those of the genome from base T0 on, with the bits outside [g0, g1) cleared (they belong to the
// pieces before and behind, which share the piece's first and last tile)
__global__ void __launch_bounds__(256) k_rep_piece_words(const uint64_t *__restrict__ all, int64_t nw, int64_t T0, int64_t g0, int64_t g1,
                                                         uint64_t *__restrict__ words) {
    const int64_t w = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (w >= nw) return;
    const int64_t B = T0 + 64 * w;
    uint64_t f = all[(T0 >> 6) + w];
    if (B < g0) f = g0 - B >= 64 ? 0 : f & (~uint64_t(0) << (g0 - B));
    if (B + 64 > g1) f = g1 <= B ? 0 : f & (~uint64_t(0) >> (B + 64 - g1));
    words[w] = f;
}

// keys for vpr_repeat_sort_floor: a hash of the index (splitmix64), and the index as the value
__global__ void __launch_bounds__(256) k_rep_random_keys(uint64_t n, uint64_t seed, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= n) return;
    uint64_t z = seed + (j + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    keys[j] = z ^ (z >> 31);
    vals[j] = uint32_t(j);
}

}  // extern "C"

// ---- KmerWork and KmerState (pr_kmer.h)

int KmerWork::check_args(vpr_handle *h, const char *entry, int min_k, int max_k, int max_spec, int32_t n_ctg, const int64_t *ctg_off,
                         const uint8_t *ctg_seq, const vpr_repeat_stratum *spec, int32_t n_spec) {
    if (!spec) return fail(h, VPR_ERR_ARG, "%s: null spec", entry);
    if (n_spec < 1 || n_spec > max_spec) return fail(h, VPR_ERR_ARG, "%s: n_spec %d is not in 1..%d", entry, n_spec, max_spec);
    for (int e = 0; e < n_spec; e++) {
        if (spec[e].k < min_k || spec[e].k > max_k)
            return fail(h, VPR_ERR_ARG, "%s: entry %d: k %d is not in %d..%d", entry, e, spec[e].k, min_k, max_k);
        if (spec[e].slop < 0) return fail(h, VPR_ERR_ARG, "%s: entry %d: slop %d is negative", entry, e, spec[e].slop);
    }
    if (n_ctg < 1 || !ctg_off) return fail(h, VPR_ERR_ARG, "%s: no contig", entry);
    if (ctg_off[0] != 0) return fail(h, VPR_ERR_ARG, "%s: ctg_off[0] is not 0", entry);
    for (int c = 0; c < n_ctg; c++) {
        const int64_t L = ctg_off[c + 1] - ctg_off[c];
        if (L < 0 || L > INT32_MAX) return fail(h, VPR_ERR_ARG, "%s: contig %d has %lld bases", entry, c, (long long)L);
    }
    const int64_t N = ctg_off[n_ctg];
    if (N > int64_t(UINT32_MAX))
        return fail(h, VPR_ERR_ARG, "%s: %lld bases in total, above the %u that 32-bit starts can name", entry, (long long)N, UINT32_MAX);
    if (N && !ctg_seq) return fail(h, VPR_ERR_ARG, "%s: null ctg_seq", entry);
    return VPR_OK;
}

int KmerWork::need(DevBuf<uint8_t> &b, size_t bytes, const char *what) {
    if (b.cap >= bytes) return VPR_OK;
    const std::string nomem = std::string(room_entry) + ": cannot allocate %zu bytes on the device (" + what + ")";
    return b.reserve(h, (bytes + 255) & ~size_t(255), nomem.c_str());
}

int KmerWork::upload(int32_t n_ctg_, const int64_t *ctg_off_, const uint8_t *ctg_seq, size_t n_rows_, int other_tile) {
    n_ctg = n_ctg_; ctg_off = ctg_off_; N = ctg_off[n_ctg]; n_rows = n_rows_;
    if (int rc = ctx_need(h, W.entry, d_off, 8 * (n_rows + 1), "row offsets")) return rc;
    if (int rc = ctx_need(h, W.entry, d_start, 4 * 1024, "intervals")) return rc;
    if (int rc = ctx_need(h, W.entry, d_stop, 4 * 1024, "intervals")) return rc;
    // the sequence, padded with zero bytes (not called) to whole tiles plus one, so that every 16-byte load of the pack stays inside
    n_tiles = (N + REP_TILE - 1) / REP_TILE; n_pad = n_tiles * REP_TILE + REP_TILE;
    nw = n_tiles * (REP_TILE / 64);
    const int64_t n_tiles_max = other_tile ? std::max(n_tiles, (N + other_tile - 1) / other_tile) : n_tiles;
    if (int rc = need(W.seq, size_t(n_pad), "contig sequences")) return rc;
    if (int rc = W.need(W.ctg_off, 8 * (size_t(n_ctg) + 1), "contig offsets")) return rc;
    if (int rc = W.need(W.small, 256, "counters")) return rc;
    if (int rc = need(flags, size_t(nw) * 8 + 8, "flag bits")) return rc;
    if (int rc = W.need(cnt, size_t(n_tiles_max + 1) * 8, "workgroup counts")) return rc;
    if (N) HIPCHK(h, hipMemcpyAsync(W.seq.p, ctg_seq, size_t(N), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(as<uint8_t>(W.seq) + N, 0, size_t(n_pad - N), h->stream));
    HIPCHK(h, hipMemcpyAsync(W.ctg_off.p, ctg_off, 8 * (size_t(n_ctg) + 1), hipMemcpyHostToDevice, h->stream));
    d_seq = as<uint8_t>(W.seq); d_ctg = as<int64_t>(W.ctg_off);
    d_count = reinterpret_cast<unsigned long long *>(as<uint8_t>(W.small) + 128);   // (the run passes use the first word)
    pieces = ctx_pieces(ctg_off, n_ctg);                                            // for the run passes, as in vpr_context_masks
    return VPR_OK;
}

int KmerWork::begin_timing(KmerState *S) {
    W.ev[0] = S->ev[0]; W.ev[1] = S->ev[1];
    HIPCHK(h, x_sync(h, h->stream, SITE));       // (the uploads and what the allocations left behind are not part of the passes' time)
    return VPR_OK;
}

int KmerWork::scan(const uint32_t *in, uint32_t *out, size_t n) {
    size_t bytes = 0;
    if (vplan_exclusive_scan_u32(nullptr, &bytes, in, out, n, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: scan workspace query failed", W.entry);
    if (int rc = W.need(W.tmp, bytes + 256, "scan workspace")) return rc;
    if (vplan_exclusive_scan_u32(W.tmp.p, &bytes, in, out, n, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: scan failed", W.entry);
    return VPR_OK;
}

int KmerWork::pair_room(size_t n) {
    if (int rc = need(keys, n * 16, "sort keys, two buffers")) return rc;
    return need(vals, n * 8, "sort values, two buffers");
}

int KmerWork::sort_room(size_t n, unsigned bits, size_t *bytes_out) {
    uint64_t *k = as<uint64_t>(keys);
    uint32_t *v = as<uint32_t>(vals);
    size_t bytes = 0;
    if (vplan_sort_pairs_u64(nullptr, &bytes, k, k + n, v, v + n, n, bits, h->stream) != 0)
        return fail(h, VPR_ERR_DEVICE, "%s: sort workspace query failed", W.entry);
    if (bytes_out) *bytes_out = bytes;
    return need(sort_tmp, bytes + 256, "sort workspace");
}

int KmerWork::sort(size_t n, unsigned bits) {
    size_t bytes = 0;
    if (int rc = sort_room(n, bits, &bytes)) return rc;
    uint64_t *k = as<uint64_t>(keys);
    uint32_t *v = as<uint32_t>(vals);
    keys_out = k + n; vals_out = v + n;
    if (vplan_sort_pairs_u64(sort_tmp.p, &bytes, k, keys_out, v, vals_out, n, bits, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: sort failed", W.entry);
    return VPR_OK;
}

int KmerWork::pack(int k, uint32_t *n, bool forward) {
    return compact(n_tiles, [&](bool write, uint32_t *out, uint64_t *ks, uint32_t *vs) {
        const auto kernel = !write ? k_rep_pack<false, false> : forward ? k_rep_pack<true, true> : k_rep_pack<true, false>;
        hipLaunchKernelGGL(kernel, dim3(unsigned(n_tiles)), dim3(REP_WG), 0, h->stream, d_seq, d_ctg, n_ctg, N, k, out, ks, vs);
    }, n);
}

int KmerWork::mark(uint32_t n, int k, unsigned long long *n_rep) {
    *n_rep = 0;
    HIPCHK(h, hipMemsetAsync(flags.p, 0, size_t(nw) * 8 + 8, h->stream));
    if (!n) return VPR_OK;
    HIPCHK(h, hipMemsetAsync(d_count + 1, 0, 8, h->stream));
    hipLaunchKernelGGL(k_rep_mark, dim3(std::min(blocks_of(int64_t(n)), MARK_MAX_WG)), dim3(256), 0, h->stream, keys_out, vals_out, uint64_t(n), k,
                       as<uint32_t>(flags), d_count + 1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(n_rep, d_count + 1, 8, hipMemcpyDeviceToHost, h->stream));
    return VPR_OK;
}

int KmerWork::rows_of_entry(int k, int slop, int spec_entry, int slot, int64_t *n_iv) {
    int64_t *row_off = d_off.p + size_t(slot) * size_t(n_ctg);
    const CtxRunRule rule = {k - 1, 1, 0, slop, 1, false};
    for (const CtxPiece &pc : pieces) {
        const int64_t g0 = ctg_off[pc.c0], g1 = ctg_off[pc.c1], T0 = g0 / REP_TILE * REP_TILE;
        const int64_t nw_pc = (g1 - T0 + REP_TILE - 1) / REP_TILE * (REP_TILE / 64);
        uint32_t n_out = 0;
        if (int rc = W.seg_begin()) return rc;
        if (nw_pc) {
            if (int rc = W.need(W.bits, size_t(nw_pc) * 8, "flag bits of a piece")) return rc;
            hipLaunchKernelGGL(k_rep_piece_words, dim3(blocks_of(nw_pc)), dim3(256), 0, h->stream, as<uint64_t>(flags), nw_pc, T0, g0, g1, as<uint64_t>(W.bits));
            HIPCHK(h, hipGetLastError());
        }
        if (int rc = ctx_intervals_from_flags(W, as<uint64_t>(W.bits), nw_pc, T0, g0, d_seq, d_ctg, n_ctg, pc.c0, pc.c1, rule, spec_entry, d_start, d_stop,
                                              size_t(*n_iv), row_off, &n_out))
            return rc;
        *n_iv += n_out;
    }
    return W.open ? W.seg_end() : VPR_OK;
}

int KmerWork::download_rows(int64_t n_iv, std::vector<int64_t> &off, std::vector<int32_t> &start, std::vector<int32_t> &stop) {
    off.assign(n_rows + 1, 0); start.assign(size_t(n_iv), 0); stop.assign(size_t(n_iv), 0);
    HIPCHK(h, hipMemcpyAsync(off.data(), d_off.p, 8 * (n_rows + 1), hipMemcpyDeviceToHost, h->stream));
    if (n_iv) {
        HIPCHK(h, hipMemcpyAsync(start.data(), d_start.p, 4 * size_t(n_iv), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(stop.data(), d_stop.p, 4 * size_t(n_iv), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    off[n_rows] = n_iv;
    return VPR_OK;
}

int KmerState::init(vpr_handle *h, int32_t n_spec_, int32_t n_ctg_) {
    for (int k = 0; k < 2; k++) HIPCHK(h, hipEventCreate(&ev[k]));
    n_spec = n_spec_; n_ctg = n_ctg_;
    n_valid.assign(size_t(n_spec), 0); n_repeated.assign(size_t(n_spec), 0);
    return VPR_OK;
}

int kmer_interval_counts(vpr_handle *h, const KmerState *S, const char *self, const char *entry, int64_t *iv_off) {
    if (!iv_off) return VPR_ERR_ARG;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "%s before %s", self, entry);
    std::copy(S->off.begin(), S->off.end(), iv_off);
    return VPR_OK;
}

int kmer_download_intervals(vpr_handle *h, const KmerState *S, const char *self, const char *entry, int32_t *start, int32_t *stop) {
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "%s before %s", self, entry);
    if (S->start.empty()) return VPR_OK;
    if (!start || !stop) return fail(h, VPR_ERR_ARG, "%s: null buffer", self);
    std::copy(S->start.begin(), S->start.end(), start);
    std::copy(S->stop.begin(), S->stop.end(), stop);
    return VPR_OK;
}

int kmer_stats(vpr_handle *h, const KmerState *S, const char *self, const char *entry, bool bufs, int64_t *n_valid, int64_t *n_repeated) {
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "%s before %s", self, entry);
    if (!bufs || !n_valid || !n_repeated) return fail(h, VPR_ERR_ARG, "%s: null buffer", self);
    std::copy(S->n_valid.begin(), S->n_valid.end(), n_valid);
    std::copy(S->n_repeated.begin(), S->n_repeated.end(), n_repeated);
    return VPR_OK;
}

int kmer_timing(const KmerState *S, double *ms0, double *ms1, double *ms2, double *ms3) {
    if (!ms0 || !ms1 || !ms2 || !ms3) return VPR_ERR_ARG;
    const bool on = S && S->valid;
    *ms0 = on ? S->ms[0] : 0; *ms1 = on ? S->ms[1] : 0; *ms2 = on ? S->ms[2] : 0; *ms3 = on ? S->ms[3] : 0;
    return VPR_OK;
}

void repeats_free(vpr_handle *h) { kmer_free(h, &vpr_handle::repeats); }

extern "C" {

int vpr_repeats_default(const vpr_repeat_stratum **spec, const char *const **names, int32_t *n) {
    if (!spec || !names || !n) return VPR_ERR_ARG;
    *spec = DEFAULT_SPEC; *names = DEFAULT_NAMES; *n = int32_t(sizeof(DEFAULT_SPEC) / sizeof(DEFAULT_SPEC[0]));
    return VPR_OK;
}

int vpr_repeat_intervals(vpr_handle *h, int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, const vpr_repeat_stratum *spec,
                         int32_t n_spec) {
    if (!h) return VPR_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    repeats_free(h);                     // the intervals of the last call end with this one, whatever becomes of it
    if (int rc = KmerWork::check_args(h, ENTRY, VPR_REP_MIN_K, VPR_REP_MAX_K, VPR_REP_MAX_SPEC, n_ctg, ctg_off, ctg_seq, spec, n_spec)) return rc;
    KmerState *S = h->repeats = new KmerState();
    if (int rc = S->init(h, n_spec, n_ctg)) return rc;
    KmerWork K(h, ENTRY);
    CtxWork &W = K.W;
    if (int rc = K.upload(n_ctg, ctg_off, ctg_seq, size_t(n_spec) * size_t(n_ctg))) return rc;
    if (int rc = K.begin_timing(S)) return rc;

    int64_t n_iv = 0;
    for (int e = 0; e < n_spec; e++) {
        const int k = spec[e].k;
        uint32_t n = 0;                  // valid starts (at most N <= UINT32_MAX)
        unsigned long long n_rep = 0;
        if (K.n_tiles) {
            W.ms = &S->ms[0];
            if (int rc = W.seg_begin()) return rc;
            if (int rc = K.pack(k, &n)) return rc;
            if (int rc = W.seg_end()) return rc;
        }
        S->n_valid[size_t(e)] = int64_t(n);
        if (n) {
            W.ms = &S->ms[1];
            if (int rc = K.sort_room(n, unsigned(2 * k))) return rc;     // (not under the sort's clock)
            if (int rc = W.seg_begin()) return rc;
            if (int rc = K.sort(n, unsigned(2 * k))) return rc;
            if (int rc = W.seg_end()) return rc;
            W.ms = &S->ms[2];
            if (int rc = W.seg_begin()) return rc;
        }
        if (int rc = K.mark(n, k, &n_rep)) return rc;                    // (without a valid start: the flags are cleared, untimed)
        if (W.open) if (int rc = W.seg_end()) return rc;
        S->n_repeated[size_t(e)] = int64_t(n_rep);
        W.ms = &S->ms[3];
        if (int rc = K.rows_of_entry(k, spec[e].slop, e, e, &n_iv)) return rc;
    }
    if (int rc = K.download_rows(n_iv, S->off, S->start, S->stop)) return rc;
    S->valid = true;
    return VPR_OK;
}

int vpr_repeat_interval_counts(vpr_handle *h, int64_t *iv_off) {
    return h ? kmer_interval_counts(h, h->repeats, "vpr_repeat_interval_counts", ENTRY, iv_off) : VPR_ERR_ARG;
}

int vpr_repeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop) {
    return h ? kmer_download_intervals(h, h->repeats, "vpr_repeat_download_intervals", ENTRY, start, stop) : VPR_ERR_ARG;
}

int vpr_repeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated) {
    return h ? kmer_stats(h, h->repeats, "vpr_repeat_stats", ENTRY, true, n_valid, n_repeated) : VPR_ERR_ARG;
}

int vpr_repeat_sort_floor(vpr_handle *h, int64_t n, int32_t k, uint64_t seed, double *ms) {
    if (!h || !ms) return VPR_ERR_ARG;
    if (n < 1 || n > int64_t(UINT32_MAX) || k < VPR_REP_MIN_K || k > VPR_REP_MAX_K)
        return fail(h, VPR_ERR_ARG, "vpr_repeat_sort_floor: n %lld or k %d outside the limits of vpr_repeat_intervals", (long long)n, k);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    KmerWork K(h, "vpr_repeat_sort_floor", ENTRY);       // (its arrays have always been refused under the name of the entry it measures)
    if (int rc = K.pair_room(size_t(n))) return rc;
    if (int rc = K.sort_room(size_t(n), unsigned(2 * k))) return rc;
    hipEvent_t ev[2];
    for (int i = 0; i < 2; i++) HIPCHK(h, hipEventCreate(&ev[i]));
    hipLaunchKernelGGL(k_rep_random_keys, dim3(blocks_of(n)), dim3(256), 0, h->stream, uint64_t(n), seed, as<uint64_t>(K.keys), as<uint32_t>(K.vals));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev[0], h->stream);
    const int rc = e == hipSuccess ? K.sort(size_t(n), unsigned(2 * k)) : VPR_OK;
    if (e == hipSuccess) e = hipEventRecord(ev[1], h->stream);
    if (e == hipSuccess) e = x_sync(h, h->stream, SITE);
    float t = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
    for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev[i]);
    if (e != hipSuccess) return fail(h, VPR_ERR_DEVICE, "vpr_repeat_sort_floor: %s", hipGetErrorString(e));
    if (rc) return rc;                   // ("vpr_repeat_sort_floor: sort failed")
    *ms = t;
    return VPR_OK;
}

int vpr_repeat_timing(const vpr_handle *h, double *ms_pack, double *ms_sort, double *ms_mark, double *ms_intervals) {
    return h ? kmer_timing(h->repeats, ms_pack, ms_sort, ms_mark, ms_intervals) : VPR_ERR_ARG;
}

}  // extern "C"
