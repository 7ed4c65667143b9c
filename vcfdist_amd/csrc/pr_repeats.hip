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
// Device memory: 1 byte per base (the sequence, resident for the call) + 1/8 byte per base (the flag bits) + 1/8 byte per base of
// the largest piece (its masked copy) + per valid start of the entry with the most 2 x 12 bytes (key and value, double-buffered
// for the sort) + rocPRIM's temporary + what the run passes take (pr_context.hip).  At most 2^32 - 1 bases: values are 32-bit.
#include "pr_host.h"
#include "pr_plan.h"
#include "pr_ctxdev.h"
#include "../../include/vcfdist_repeats.h"

struct RepeatState {
    int32_t n_spec = 0, n_ctg = 0;
    int64_t n_iv = 0;
    DevBuf<int64_t> d_off;                             // [n_spec * n_ctg + 1]
    DevBuf<int32_t> d_start, d_stop;                   // [n_iv]
    std::vector<int64_t> n_valid, n_repeated;          // [n_spec]
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_pack = 0, ms_sort = 0, ms_mark = 0, ms_intervals = 0;
    bool valid = false;
};

namespace {

const int REP_LANE = 16, REP_WG = 256, REP_TILE = REP_LANE * REP_WG;      // the pack kernels: starts of a lane / a workgroup
const int REP_HALO = VPR_REP_MAX_K - 1;                                    // bases behind a lane's 16 that its last start reads
const unsigned MARK_MAX_WG = 4096;                                         // workgroups of the mark kernel (k_rep_mark)
const int REP_WORDS = (REP_LANE + REP_HALO + 15) / 16 * 4;                 // the lane's bytes as 32-bit words: three 16-byte loads

const vpr_repeat_stratum DEFAULT_SPEC[] = {{16, 0}, {24, 0}, {32, 0}};
const char *const DEFAULT_NAMES[] = {"rep_k16", "rep_k24", "rep_k32"};
const char *const ENTRY = "vpr_repeat_intervals";

// The starts G .. G + 15 of one lane, whose bytes [G, G + 48) are in w: returns how many are valid and, with EMIT, writes their
// (canon, start) from keys[at] / vals[at] on in start order.  Base G + jj is consumed at step jj; the k-mer that ends there starts
// at G + jj - (k - 1) and is valid iff the last k bases consumed were called and no contig began behind the first of them.
template <bool EMIT>
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
            if (EMIT) { keys[at + n] = fwd < rc ? fwd : rc; vals[at + n] = uint32_t(Gp - (k - 1)); }
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
template <bool WRITE>
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
        if (n) (void)rep_roll<true>(w, G, ctg_off, n_ctg, k, tile_keys, tile_vals, before);      // (before + n <= total <= REP_TILE)
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

namespace {

template <typename T>
T *as(const DevBuf<uint8_t> &b) { return reinterpret_cast<T *>(b.p); }

// room for exactly `bytes` (the arrays that scale with the genome are not given the quarter more of ctx_need)
int rep_need(vpr_handle *h, DevBuf<uint8_t> &b, size_t bytes, const char *what) {
    if (b.cap >= bytes) return VPR_OK;
    const std::string nomem = std::string(ENTRY) + ": cannot allocate %zu bytes on the device (" + what + ")";
    return b.reserve(h, (bytes + 255) & ~size_t(255), nomem.c_str());
}

struct RepBufs {                         // the genome-wide arrays of the call, released when it goes
    vpr_handle *h;
    DevBuf<uint8_t> flags, cnt, keys, vals, sort_tmp;
    explicit RepBufs(vpr_handle *h_) : h(h_) {}
    ~RepBufs() {
        (void)hipStreamSynchronize(h->stream);
        dev_release(h, flags, cnt, keys, vals, sort_tmp);
    }
};

unsigned blocks_of(int64_t n) { return unsigned((n + 255) / 256); }

}  // namespace

void repeats_free(vpr_handle *h) {
    RepeatState *S = h->repeats;
    if (!S) return;
    (void)hipStreamSynchronize(h->stream);
    dev_release(h, S->d_off, S->d_start, S->d_stop);
    for (int k = 0; k < 2; k++) if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
    delete S;
    h->repeats = nullptr;
}

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
    // every check comes before a byte of ctg_seq is read
    if (!spec) return fail(h, VPR_ERR_ARG, "%s: null spec", ENTRY);
    if (n_spec < 1 || n_spec > VPR_REP_MAX_SPEC) return fail(h, VPR_ERR_ARG, "%s: n_spec %d is not in 1..%d", ENTRY, n_spec, VPR_REP_MAX_SPEC);
    for (int e = 0; e < n_spec; e++) {
        if (spec[e].k < VPR_REP_MIN_K || spec[e].k > VPR_REP_MAX_K)
            return fail(h, VPR_ERR_ARG, "%s: entry %d: k %d is not in %d..%d", ENTRY, e, spec[e].k, VPR_REP_MIN_K, VPR_REP_MAX_K);
        if (spec[e].slop < 0) return fail(h, VPR_ERR_ARG, "%s: entry %d: slop %d is negative", ENTRY, e, spec[e].slop);
    }
    if (n_ctg < 1 || !ctg_off) return fail(h, VPR_ERR_ARG, "%s: no contig", ENTRY);
    if (ctg_off[0] != 0) return fail(h, VPR_ERR_ARG, "%s: ctg_off[0] is not 0", ENTRY);
    for (int c = 0; c < n_ctg; c++) {
        const int64_t L = ctg_off[c + 1] - ctg_off[c];
        if (L < 0 || L > INT32_MAX) return fail(h, VPR_ERR_ARG, "%s: contig %d has %lld bases", ENTRY, c, (long long)L);
    }
    const int64_t N = ctg_off[n_ctg];
    if (N > int64_t(UINT32_MAX))
        return fail(h, VPR_ERR_ARG, "%s: %lld bases in total, above the %u that 32-bit starts can name", ENTRY, (long long)N, UINT32_MAX);
    if (N && !ctg_seq) return fail(h, VPR_ERR_ARG, "%s: null ctg_seq", ENTRY);

    RepeatState *S = h->repeats = new RepeatState();
    for (int k = 0; k < 2; k++) HIPCHK(h, hipEventCreate(&S->ev[k]));
    S->n_spec = n_spec; S->n_ctg = n_ctg;
    S->n_valid.assign(size_t(n_spec), 0); S->n_repeated.assign(size_t(n_spec), 0);
    const size_t rows = size_t(n_spec) * size_t(n_ctg);
    if (int rc = ctx_need(h, ENTRY, S->d_off, 8 * (rows + 1), "row offsets")) return rc;
    if (int rc = ctx_need(h, ENTRY, S->d_start, 4 * 1024, "intervals")) return rc;
    if (int rc = ctx_need(h, ENTRY, S->d_stop, 4 * 1024, "intervals")) return rc;

    CtxWork W(h, ENTRY);
    RepBufs R(h);
    // the sequence, padded with zero bytes (not called) to whole tiles plus one, so that every 16-byte load stays inside
    const int64_t n_tiles_all = (N + REP_TILE - 1) / REP_TILE, n_pad = n_tiles_all * REP_TILE + REP_TILE;
    const int64_t nw_all = n_tiles_all * (REP_TILE / 64);                   // 64-bit flag words of the genome
    if (int rc = rep_need(h, W.seq, size_t(n_pad), "contig sequences")) return rc;
    if (int rc = W.need(W.ctg_off, 8 * (size_t(n_ctg) + 1), "contig offsets")) return rc;
    if (int rc = W.need(W.small, 256, "counters")) return rc;
    if (int rc = rep_need(h, R.flags, size_t(nw_all) * 8 + 8, "flag bits")) return rc;
    if (int rc = W.need(R.cnt, size_t(n_tiles_all + 1) * 8, "workgroup counts")) return rc;
    if (N) HIPCHK(h, hipMemcpyAsync(W.seq.p, ctg_seq, size_t(N), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(as<uint8_t>(W.seq) + N, 0, size_t(n_pad - N), h->stream));
    HIPCHK(h, hipMemcpyAsync(W.ctg_off.p, ctg_off, 8 * (size_t(n_ctg) + 1), hipMemcpyHostToDevice, h->stream));
    const uint8_t *d_seq = as<uint8_t>(W.seq);
    const int64_t *d_ctg = as<int64_t>(W.ctg_off);
    uint32_t *cnt = as<uint32_t>(R.cnt), *off = cnt + (n_tiles_all + 1);
    unsigned long long *d_nrep = reinterpret_cast<unsigned long long *>(as<uint8_t>(W.small) + 128);   // (the run passes use the first word)

    // pieces of whole contigs for the run passes, as in vpr_context_masks
    struct Piece { int c0, c1; };       // contigs [c0, c1)
    std::vector<Piece> pieces;
    const int64_t budget = ctx_piece_bases();
    for (int c = 0; c < n_ctg;) {
        int e = c + 1;
        while (e < n_ctg && ctg_off[e + 1] - ctg_off[c] <= budget) e++;
        pieces.push_back({c, e});
        c = e;
    }

    W.ev[0] = S->ev[0]; W.ev[1] = S->ev[1];
    HIPCHK(h, x_sync(h, h->stream, SITE));       // (the uploads are not part of the passes' time)

    int64_t n_iv = 0;
    for (int e = 0; e < n_spec; e++) {
        const int k = spec[e].k;
        uint32_t n = 0;                  // valid starts (at most N <= UINT32_MAX)
        if (n_tiles_all) {
            W.ms = &S->ms_pack;
            if (int rc = W.seg_begin()) return rc;
            HIPCHK(h, hipMemsetAsync(cnt + n_tiles_all, 0, 4, h->stream));
            hipLaunchKernelGGL(k_rep_pack<false>, dim3(unsigned(n_tiles_all)), dim3(REP_WG), 0, h->stream, d_seq, d_ctg, n_ctg, N, k, cnt,
                               (uint64_t *)nullptr, (uint32_t *)nullptr);
            HIPCHK(h, hipGetLastError());
            {
                size_t bytes = 0;
                if (vplan_exclusive_scan_u32(nullptr, &bytes, cnt, off, size_t(n_tiles_all + 1), h->stream) != 0)
                    return fail(h, VPR_ERR_DEVICE, "%s: scan workspace query failed", ENTRY);
                if (int rc = W.need(W.tmp, bytes + 256, "scan workspace")) return rc;
                if (vplan_exclusive_scan_u32(W.tmp.p, &bytes, cnt, off, size_t(n_tiles_all + 1), h->stream) != 0)
                    return fail(h, VPR_ERR_DEVICE, "%s: scan failed", ENTRY);
            }
            HIPCHK(h, hipMemcpyAsync(&n, off + n_tiles_all, 4, hipMemcpyDeviceToHost, h->stream));
            if (int rc = W.seg_end()) return rc;
        }
        S->n_valid[size_t(e)] = int64_t(n);
        if (n) {
            if (int rc = rep_need(h, R.keys, size_t(n) * 16, "sort keys, two buffers")) return rc;
            if (int rc = rep_need(h, R.vals, size_t(n) * 8, "sort values, two buffers")) return rc;
            uint64_t *keys = as<uint64_t>(R.keys), *keys_out = keys + n;
            uint32_t *vals = as<uint32_t>(R.vals), *vals_out = vals + n;
            if (int rc = W.seg_begin()) return rc;
            hipLaunchKernelGGL(k_rep_pack<true>, dim3(unsigned(n_tiles_all)), dim3(REP_WG), 0, h->stream, d_seq, d_ctg, n_ctg, N, k, off, keys, vals);
            HIPCHK(h, hipGetLastError());
            if (int rc = W.seg_end()) return rc;

            W.ms = &S->ms_sort;
            size_t bytes = 0;
            if (vplan_sort_pairs_u64(nullptr, &bytes, keys, keys_out, vals, vals_out, size_t(n), unsigned(2 * k), h->stream) != 0)
                return fail(h, VPR_ERR_DEVICE, "%s: sort workspace query failed", ENTRY);
            if (int rc = rep_need(h, R.sort_tmp, bytes + 256, "sort workspace")) return rc;
            if (int rc = W.seg_begin()) return rc;
            if (vplan_sort_pairs_u64(R.sort_tmp.p, &bytes, keys, keys_out, vals, vals_out, size_t(n), unsigned(2 * k), h->stream) != 0)
                return fail(h, VPR_ERR_DEVICE, "%s: sort failed", ENTRY);
            if (int rc = W.seg_end()) return rc;

            W.ms = &S->ms_mark;
            unsigned long long n_rep = 0;
            if (int rc = W.seg_begin()) return rc;
            HIPCHK(h, hipMemsetAsync(R.flags.p, 0, size_t(nw_all) * 8 + 8, h->stream));
            HIPCHK(h, hipMemsetAsync(d_nrep, 0, 8, h->stream));
            hipLaunchKernelGGL(k_rep_mark, dim3(std::min(blocks_of(int64_t(n)), MARK_MAX_WG)), dim3(256), 0, h->stream, keys_out, vals_out, uint64_t(n), k,
                               as<uint32_t>(R.flags), d_nrep);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(&n_rep, d_nrep, 8, hipMemcpyDeviceToHost, h->stream));
            if (int rc = W.seg_end()) return rc;
            S->n_repeated[size_t(e)] = int64_t(n_rep);
        } else {
            HIPCHK(h, hipMemsetAsync(R.flags.p, 0, size_t(nw_all) * 8 + 8, h->stream));
        }

        W.ms = &S->ms_intervals;
        int64_t *row_off = S->d_off.p + size_t(e) * size_t(n_ctg);
        const CtxRunRule rule = {k - 1, 1, 0, spec[e].slop, 1, false};
        for (const Piece &pc : pieces) {
            const int64_t g0 = ctg_off[pc.c0], g1 = ctg_off[pc.c1], T0 = g0 / REP_TILE * REP_TILE;
            const int64_t n_tiles = (g1 - T0 + REP_TILE - 1) / REP_TILE, nw = n_tiles * (REP_TILE / 64);
            uint32_t n_out = 0;
            if (int rc = W.seg_begin()) return rc;
            if (nw) {
                if (int rc = W.need(W.bits, size_t(nw) * 8, "flag bits of a piece")) return rc;
                hipLaunchKernelGGL(k_rep_piece_words, dim3(blocks_of(nw)), dim3(256), 0, h->stream, as<uint64_t>(R.flags), nw, T0, g0, g1,
                                   as<uint64_t>(W.bits));
                HIPCHK(h, hipGetLastError());
            }
            if (int rc = ctx_intervals_from_flags(W, as<uint64_t>(W.bits), nw, T0, g0, d_seq, d_ctg, n_ctg, pc.c0, pc.c1, rule, e, S->d_start, S->d_stop,
                                                  size_t(n_iv), row_off, &n_out))
                return rc;
            n_iv += n_out;
        }
        if (W.open) if (int rc = W.seg_end()) return rc;
    }
    S->n_iv = n_iv;
    S->valid = true;
    return VPR_OK;
}

int vpr_repeat_interval_counts(vpr_handle *h, int64_t *iv_off) {
    if (!h || !iv_off) return VPR_ERR_ARG;
    const RepeatState *S = h->repeats;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_repeat_interval_counts before vpr_repeat_intervals");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t rows = size_t(S->n_spec) * size_t(S->n_ctg);
    HIPCHK(h, hipMemcpyAsync(iv_off, S->d_off.p, 8 * (rows + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    return VPR_OK;
}

int vpr_repeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop) {
    if (!h) return VPR_ERR_ARG;
    const RepeatState *S = h->repeats;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_repeat_download_intervals before vpr_repeat_intervals");
    if (!S->n_iv) return VPR_OK;
    if (!start || !stop) return fail(h, VPR_ERR_ARG, "vpr_repeat_download_intervals: null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(start, S->d_start.p, 4 * size_t(S->n_iv), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(stop, S->d_stop.p, 4 * size_t(S->n_iv), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    return VPR_OK;
}

int vpr_repeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated) {
    if (!h) return VPR_ERR_ARG;
    const RepeatState *S = h->repeats;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_repeat_stats before vpr_repeat_intervals");
    if (!n_valid || !n_repeated) return fail(h, VPR_ERR_ARG, "vpr_repeat_stats: null buffer");
    for (int e = 0; e < S->n_spec; e++) { n_valid[e] = S->n_valid[size_t(e)]; n_repeated[e] = S->n_repeated[size_t(e)]; }
    return VPR_OK;
}

int vpr_repeat_sort_floor(vpr_handle *h, int64_t n, int32_t k, uint64_t seed, double *ms) {
    if (!h || !ms) return VPR_ERR_ARG;
    if (n < 1 || n > int64_t(UINT32_MAX) || k < VPR_REP_MIN_K || k > VPR_REP_MAX_K)
        return fail(h, VPR_ERR_ARG, "vpr_repeat_sort_floor: n %lld or k %d outside the limits of vpr_repeat_intervals", (long long)n, k);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    RepBufs R(h);
    if (int rc = rep_need(h, R.keys, size_t(n) * 16, "sort keys, two buffers")) return rc;
    if (int rc = rep_need(h, R.vals, size_t(n) * 8, "sort values, two buffers")) return rc;
    uint64_t *keys = as<uint64_t>(R.keys), *keys_out = keys + n;
    uint32_t *vals = as<uint32_t>(R.vals), *vals_out = vals + n;
    size_t bytes = 0;
    if (vplan_sort_pairs_u64(nullptr, &bytes, keys, keys_out, vals, vals_out, size_t(n), unsigned(2 * k), h->stream) != 0)
        return fail(h, VPR_ERR_DEVICE, "vpr_repeat_sort_floor: sort workspace query failed");
    if (int rc = rep_need(h, R.sort_tmp, bytes + 256, "sort workspace")) return rc;
    hipEvent_t ev[2];
    for (int i = 0; i < 2; i++) HIPCHK(h, hipEventCreate(&ev[i]));
    hipLaunchKernelGGL(k_rep_random_keys, dim3(blocks_of(n)), dim3(256), 0, h->stream, uint64_t(n), seed, keys, vals);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev[0], h->stream);
    const int rc = e == hipSuccess ? vplan_sort_pairs_u64(R.sort_tmp.p, &bytes, keys, keys_out, vals, vals_out, size_t(n), unsigned(2 * k), h->stream) : 0;
    if (e == hipSuccess) e = hipEventRecord(ev[1], h->stream);
    if (e == hipSuccess) e = x_sync(h, h->stream, SITE);
    float t = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
    for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev[i]);
    if (e != hipSuccess) return fail(h, VPR_ERR_DEVICE, "vpr_repeat_sort_floor: %s", hipGetErrorString(e));
    if (rc != 0) return fail(h, VPR_ERR_DEVICE, "vpr_repeat_sort_floor: sort failed");
    *ms = t;
    return VPR_OK;
}

int vpr_repeat_timing(const vpr_handle *h, double *ms_pack, double *ms_sort, double *ms_mark, double *ms_intervals) {
    if (!h || !ms_pack || !ms_sort || !ms_mark || !ms_intervals) return VPR_ERR_ARG;
    const RepeatState *S = h->repeats;
    if (!S || !S->valid) { *ms_pack = *ms_sort = *ms_mark = *ms_intervals = 0; return VPR_OK; }
    *ms_pack = S->ms_pack; *ms_sort = S->ms_sort; *ms_mark = S->ms_mark; *ms_intervals = S->ms_intervals;
    return VPR_OK;
}

}  // extern "C"

// the launches pr_longrepeats.hip borrows for its base level (k = 32) and its last level (pr_host.h)
static_assert(REP_TILE == REP_PACK_TILE, "pr_host.h names the pack's tile");

void rep_launch_pack(hipStream_t st, bool write, unsigned n_tiles, const uint8_t *seq, const int64_t *ctg_off, int n_ctg, int64_t N, int k,
                     uint32_t *out, uint64_t *keys, uint32_t *vals) {
    if (write) hipLaunchKernelGGL(k_rep_pack<true>, dim3(n_tiles), dim3(REP_WG), 0, st, seq, ctg_off, n_ctg, N, k, out, keys, vals);
    else hipLaunchKernelGGL(k_rep_pack<false>, dim3(n_tiles), dim3(REP_WG), 0, st, seq, ctg_off, n_ctg, N, k, out, keys, vals);
}

void rep_launch_mark(hipStream_t st, const uint64_t *keys, const uint32_t *vals, uint64_t n, int k, uint32_t *flags32, unsigned long long *n_rep) {
    hipLaunchKernelGGL(k_rep_mark, dim3(std::min(blocks_of(int64_t(n)), MARK_MAX_WG)), dim3(256), 0, st, keys, vals, n, k, flags32, n_rep);
}

void rep_launch_piece_words(hipStream_t st, const uint64_t *all, int64_t nw, int64_t T0, int64_t g0, int64_t g1, uint64_t *words) {
    hipLaunchKernelGGL(k_rep_piece_words, dim3(blocks_of(nw)), dim3(256), 0, st, all, nw, T0, g0, g1, words);
}
