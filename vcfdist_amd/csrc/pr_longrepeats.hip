// pr_longrepeats.hip -- the long repeat strata (include/vcfdist_longrepeats.h): sorted interval lists per (stratum, contig) of the
// bases covered by a k-mer of 33 to 256 bases that occurs more than once in the genome, on either strand.
//
// A canonical k-mer above 32 bases does not fit one 64-bit sort key.  Only equality classes matter, so a k-mer is named by the
// ranks of two shorter words that cover it, and the 64-bit sort of pr_plan.hip does for every length (rank doubling).  For a length
// a every global start g has two 32-bit ids: F_a[g] of the a-mer at g, R_a[g] of its reverse complement, (class rank << 1) |
// orientation with orientation 0 where the forward a-mer is the canonical one; R == F for a reverse palindrome, else R == F ^ 1.
// Two oriented a-mers are equal exactly when their ids are.  A start that is not kept holds LR_NONE.
//   base level, a = 32   the pack of pr_repeats.hip at k = 32 and the sort over 64 key bits; k_lrep_heads (class heads of the
//                        kept classes), a scan (dense ranks), k_lrep_ids (scatter of F_32, R_32)
//   level a -> b         a < b <= 2a, d = b - a: k_lrep_pairs<false>, a scan, k_lrep_pairs<true> write (key, g) of the candidates
//                        -- F_a[g] and F_a[g + d] both kept, and with d == a both in one contig: the a-mer at g may end where the
//                        next contig begins -- compactly at prefix sums (through LDS, no atomic cursor: two calls give identical
//                        arrays); key = min((F_a[g] << 32) | F_a[g + d], (R_a[g + d] << 32) | R_a[g]), the second operand being
//                        the reverse complement's pair; the b-mer is a palindrome iff the operands are equal, and its orientation
//                        is which one won.  One sort over the bits in use, then heads, ranks and ids as at the base level.
//   schedule             32 -> 64 -> 128 -> k without the levels above k; the base level and the levels 64 and 128 are computed
//                        once per call and shared: the entries run in the order of their k and the rows are put back in the
//                        caller's order at the end
//   last level           pairs and sort as above, then k_rep_mark (pr_repeats.hip): flag bit at g + k - 1, the count of repeated
//                        starts; k_rep_piece_words and ctx_intervals_from_flags with the rule {k - 1, 1, 0, slop, 1, false}
// The filter.  An inner level keeps an a-mer iff its canonical class has at least two starts OR it is a reverse palindrome.
// "Repeated" alone is wrong: a reverse palindrome of b + d bases placed once has two repeated b-mers, at g - d and g, whose shared
// a-mer at g is its own reverse complement and may occur nowhere else.  It suffices: if the partner of the b-mer at g is the
// reverse complement at g', the a-mer at g equals the reverse complement of the a-mer at g' + d; either g' + d != g (two starts)
// or g' + d == g (a palindrome); the same at g + d; a same-strand partner gives two starts at once.  Kept classes are at most half
// the kept starts plus the palindromic singletons; 2^31 - 1 or more of them at a level is refused with the level and the count.
// n_valid of an entry is a pass of its own over the called runs (k_lrep_valid): the unrolled halo of the pack ends at 31.
//
// Device memory, with N the bases padded to whole tiles of 4096 plus one tile: N bytes (the sequence) + N / 8 (the flag bits) +
// 16 N (four id arrays: F and R of the level read and of the level written) + per valid 32-mer start 2 x 12 bytes (the base
// level's key and value, double-buffered for the sort) and 8 bytes (class heads and their scan); the upper levels use the same
// buffers for their candidates only + the tiles' counts + rocPRIM's temporary + what the run passes take (pr_context.hip).
#include "pr_host.h"
#include "pr_plan.h"
#include "pr_ctxdev.h"
#include "../../include/vcfdist_longrepeats.h"

struct LongRepeatState {
    int32_t n_spec = 0, n_ctg = 0;
    std::vector<int64_t> off;                          // [n_spec * n_ctg + 1], rows in the caller's order
    std::vector<int32_t> start, stop;                  // [off.back()]
    std::vector<int64_t> n_valid, n_repeated, n_last;  // [n_spec]
    int64_t n_level[3] = {0, 0, 0};                    // pairs sorted by the base level, the level 64 and the level 128
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_base = 0, ms_levels = 0, ms_last = 0, ms_intervals = 0;
    bool valid = false;
};

namespace {

const uint32_t LR_NONE = 0xFFFFFFFFu;                  // the id of a start that is not kept (a rank is below 2^31 - 1)
const int LR_ROUNDS = 8, LR_TILE = LR_ROUNDS * 256;    // starts of a workgroup of k_lrep_pairs, 256 a round
const int LR_ENDS = 64;                                // k-mer ends of a lane of k_lrep_valid
const int LR_BASE = 32;                                // the base level's length

const vpr_repeat_stratum DEFAULT_SPEC[] = {{64, 0}, {100, 0}, {250, 0}};
const char *const DEFAULT_NAMES[] = {"rep_k64", "rep_k100", "rep_k250"};
const char *const ENTRY = "vpr_longrepeat_intervals";

// the code of the reverse complement of a 32-mer's code: every 2-bit group complemented, the groups in reverse order
__device__ inline uint64_t rc32(uint64_t x) {
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}

// the pair of the b-mer at g and the pair of its reverse complement (halves swapped and flipped)
__device__ inline void pair_of(const uint32_t *__restrict__ F, const uint32_t *__restrict__ R, uint64_t g, int d, uint64_t *fw, uint64_t *rc) {
    *fw = uint64_t(F[g]) << 32 | F[g + d];
    *rc = uint64_t(R[g + d]) << 32 | R[g];
}

}  // namespace

// The candidates of a level a -> a + d among the starts [0, N): WRITE false, the workgroup's count into out[blockIdx.x]; WRITE true,
// out holds the exclusive scan of the counts and the workgroup's (key, start) go behind its offset in start order.  A round takes
// 256 consecutive starts, so F[g] and F[g + d] are two coalesced streams; the pairs are collected in LDS and copied out with
// consecutive lanes on consecutive elements.  The id arrays hold LR_NONE behind the genome (at least d elements are there).
template <bool WRITE>
__global__ void __launch_bounds__(256) k_lrep_pairs(const uint32_t *__restrict__ F, const uint32_t *__restrict__ R, const int64_t *__restrict__ ctg_off,
                                                    int n_ctg, int64_t N, int d, int seam, uint32_t *__restrict__ out, uint64_t *__restrict__ keys,
                                                    uint32_t *__restrict__ vals) {
    __shared__ uint32_t lds[4];
    __shared__ uint64_t tile_keys[WRITE ? LR_TILE : 1];
    __shared__ uint32_t tile_vals[WRITE ? LR_TILE : 1];
    uint32_t have = 0;
#pragma unroll 1
    for (int r = 0; r < LR_ROUNDS; r++) {
        const int64_t g = int64_t(blockIdx.x) * LR_TILE + r * 256 + threadIdx.x;
        bool cand = false;
        if (g < N) {
            cand = F[g] != LR_NONE && F[g + d] != LR_NONE;
            if (cand && seam) {              // d == a: the second half begins where the first ends, which may be another contig
                const int c = ctg_of(ctg_off, n_ctg, g);
                cand = g + d < ctg_off[c + 1];
            }
        }
        uint32_t total;
        const uint32_t before = block_scan(cand ? 1u : 0u, lds, &total);
        if constexpr (WRITE) {
            if (cand) {
                uint64_t fw, rc;
                pair_of(F, R, uint64_t(g), d, &fw, &rc);
                tile_keys[have + before] = fw < rc ? fw : rc;
                tile_vals[have + before] = uint32_t(g);
            }
        }
        have += total;
    }
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) out[blockIdx.x] = have;
    } else {
        __syncthreads();
        const uint32_t at = out[blockIdx.x];
        for (uint32_t i = threadIdx.x; i < have; i += 256) { keys[at + i] = tile_keys[i]; vals[at + i] = tile_vals[i]; }
    }
}

extern "C" {

// heads[j] = sorted element j is the first of a class that is kept: one with at least two starts, or a reverse palindrome (F null:
// the base level, whose keys are canonical codes; else the level a -> a + d, whose pairs are read again); heads[n] = 0 for the scan
__global__ void __launch_bounds__(256) k_lrep_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n,
                                                    const uint32_t *__restrict__ F, const uint32_t *__restrict__ R, int d, uint32_t *__restrict__ heads) {
    const uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j > n) return;
    bool keep = false;
    if (j < n) {
        const uint64_t key = keys[j];
        if (j == 0 || keys[j - 1] != key) {
            keep = j + 1 < n && keys[j + 1] == key;
            if (!keep) {
                if (F) { uint64_t fw, rc; pair_of(F, R, vals[j], d, &fw, &rc); keep = fw == rc; }
                else keep = rc32(key) == key;
            }
        }
    }
    heads[j] = keep ? 1u : 0u;
}

// the ids of the level written: sorted element j of a kept class has the rank scan[j + 1] - 1 (the kept heads up to and with its
// own); its orientation is read from the pair (Fa non-null) or, at the base level, from the one base of the sequence at which the
// canonical code and its reverse complement first differ.  Fb and Rb hold LR_NONE everywhere before.
__global__ void __launch_bounds__(256) k_lrep_ids(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n,
                                                  const uint32_t *__restrict__ scan, const uint32_t *__restrict__ Fa, const uint32_t *__restrict__ Ra,
                                                  int d, const uint8_t *__restrict__ seq, uint32_t *__restrict__ Fb, uint32_t *__restrict__ Rb) {
    const uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= n) return;
    const uint64_t key = keys[j];
    const bool many = (j > 0 && keys[j - 1] == key) || (j + 1 < n && keys[j + 1] == key);
    const uint64_t g = vals[j];
    bool pal;
    uint32_t orient;
    if (Fa) {
        uint64_t fw, rc;
        pair_of(Fa, Ra, g, d, &fw, &rc);
        pal = fw == rc; orient = fw > rc;
    } else {
        const uint64_t other = rc32(key);
        pal = other == key; orient = 0;
        if (!pal) {
            const int at = __builtin_clzll(key ^ other) >> 1;                  // the first base at which the two words differ
            const unsigned x = seq[g + at];
            orient = (((x >> 1) ^ (x >> 2)) & 3u) != unsigned((key >> (62 - 2 * at)) & 3u);
        }
    }
    if (!many && !pal) return;
    const uint32_t id = (scan[j + 1] - 1) << 1 | orient;
    Fb[g] = id;
    Rb[g] = pal ? id : id ^ 1u;
}

// the valid starts of length k: a lane takes LR_ENDS k-mer ends, counts the called bases in front of its first (at most k - 1 are
// of interest, and none in front of the contig's start) and walks on as rep_roll does; one add per workgroup
__global__ void __launch_bounds__(256) k_lrep_valid(const uint8_t *__restrict__ seq, const int64_t *__restrict__ ctg_off, int n_ctg, int64_t N, int k,
                                                    unsigned long long *__restrict__ n_valid) {
    __shared__ uint32_t lds[4];
    const int64_t E = (int64_t(blockIdx.x) * 256 + threadIdx.x) * LR_ENDS;
    uint32_t mine = 0;
    if (E < N) {
        int c = ctg_of(ctg_off, n_ctg, E);
        int64_t ce = ctg_off[c + 1];
        const int64_t cs = ctg_off[c], lo = E - (k - 1) > cs ? E - (k - 1) : cs;
        int run = 0;
        for (int64_t p = E - 1; p >= lo && called(seq[p]); p--) run++;
        const int64_t stop = E + LR_ENDS < N ? E + LR_ENDS : N;
        for (int64_t e = E; e < stop; e++) {
            if (e >= ce) {
                run = 0;
                while (e >= ce && c + 1 < n_ctg) { c++; ce = ctg_off[c + 1]; }
            }
            run = called(seq[e]) ? run + 1 : 0;
            mine += run >= k;
        }
    }
    uint32_t total;
    (void)block_scan(mine, lds, &total);
    if (threadIdx.x == 0 && total) atomicAdd(n_valid, (unsigned long long)total);
}

}  // extern "C"

namespace {

template <typename T>
T *as(const DevBuf<uint8_t> &b) { return reinterpret_cast<T *>(b.p); }

// room for exactly `bytes` (the arrays that scale with the genome are not given the quarter more of ctx_need)
int lrep_need(vpr_handle *h, DevBuf<uint8_t> &b, size_t bytes, const char *what) {
    if (b.cap >= bytes) return VPR_OK;
    const std::string nomem = std::string(ENTRY) + ": cannot allocate %zu bytes on the device (" + what + ")";
    return b.reserve(h, (bytes + 255) & ~size_t(255), nomem.c_str());
}

unsigned blocks_of(int64_t n) { return unsigned((n + 255) / 256); }

struct Ids { uint32_t *F, *R; uint32_t n_cls; };       // a level's id arrays and the kept classes they name

// The genome-wide arrays of one call (released when it goes) and the passes over them.
struct LongWork {
    vpr_handle *h;
    CtxWork &W;
    DevBuf<uint8_t> flags, cnt, keys, vals, sort_tmp, heads, ids;
    const uint8_t *d_seq = nullptr;
    const int64_t *d_ctg = nullptr;
    int n_ctg = 0;
    int64_t N = 0, n_pad = 0;
    unsigned long long *d_count = nullptr;
    uint64_t *keys_out = nullptr;        // the sorted pairs of the last sort
    uint32_t *vals_out = nullptr;
    LongWork(vpr_handle *h_, CtxWork &W_) : h(h_), W(W_) {}
    ~LongWork() {
        (void)hipStreamSynchronize(h->stream);
        dev_release(h, flags, cnt, keys, vals, sort_tmp, heads, ids);
    }
    Ids slot(int s) const { return {as<uint32_t>(ids) + size_t(2 * s) * size_t(n_pad), as<uint32_t>(ids) + size_t(2 * s + 1) * size_t(n_pad), 0}; }

    int scan(const uint32_t *in, uint32_t *out, size_t n) {
        size_t bytes = 0;
        if (vplan_exclusive_scan_u32(nullptr, &bytes, in, out, n, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: scan workspace query failed", ENTRY);
        if (int rc = W.need(W.tmp, bytes + 256, "scan workspace")) return rc;
        if (vplan_exclusive_scan_u32(W.tmp.p, &bytes, in, out, n, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: scan failed", ENTRY);
        return VPR_OK;
    }
    int pair_room(size_t n) {
        if (int rc = lrep_need(h, keys, n * 16, "sort keys, two buffers")) return rc;
        return lrep_need(h, vals, n * 8, "sort values, two buffers");
    }
    // the n pairs at the front of keys / vals, sorted over key bits [0, bits) into keys_out / vals_out
    int sort(size_t n, unsigned bits) {
        uint64_t *k = as<uint64_t>(keys);
        uint32_t *v = as<uint32_t>(vals);
        keys_out = k + n; vals_out = v + n;
        size_t bytes = 0;
        if (vplan_sort_pairs_u64(nullptr, &bytes, k, keys_out, v, vals_out, n, bits, h->stream) != 0)
            return fail(h, VPR_ERR_DEVICE, "%s: sort workspace query failed", ENTRY);
        if (int rc = lrep_need(h, sort_tmp, bytes + 256, "sort workspace")) return rc;
        if (vplan_sort_pairs_u64(sort_tmp.p, &bytes, k, keys_out, v, vals_out, n, bits, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: sort failed", ENTRY);
        return VPR_OK;
    }
    // the candidates of the level from -> from + d, sorted; *n_out of them.  A timed segment is under way on entry and on return.
    int pairs(const Ids &from, int a, int d, uint32_t *n_out) {
        *n_out = 0;
        if (!from.n_cls) return VPR_OK;  // (nothing is kept: no start has two kept halves)
        const int64_t n_tiles = (N + LR_TILE - 1) / LR_TILE;
        uint32_t *c = as<uint32_t>(cnt), *off = c + (n_tiles + 1);
        uint32_t n = 0;
        HIPCHK(h, hipMemsetAsync(c + n_tiles, 0, 4, h->stream));
        hipLaunchKernelGGL(k_lrep_pairs<false>, dim3(unsigned(n_tiles)), dim3(256), 0, h->stream, from.F, from.R, d_ctg, n_ctg, N, d, int(d == a), c,
                           (uint64_t *)nullptr, (uint32_t *)nullptr);
        HIPCHK(h, hipGetLastError());
        if (int rc = scan(c, off, size_t(n_tiles + 1))) return rc;
        HIPCHK(h, hipMemcpyAsync(&n, off + n_tiles, 4, hipMemcpyDeviceToHost, h->stream));
        if (int rc = W.seg_end()) return rc;
        if (n) if (int rc = pair_room(n)) return rc;
        if (int rc = W.seg_begin()) return rc;
        if (!n) return VPR_OK;
        hipLaunchKernelGGL(k_lrep_pairs<true>, dim3(unsigned(n_tiles)), dim3(256), 0, h->stream, from.F, from.R, d_ctg, n_ctg, N, d, int(d == a), off,
                           as<uint64_t>(keys), as<uint32_t>(vals));
        HIPCHK(h, hipGetLastError());
        unsigned bits = 33;              // the upper half is an id below 2 n_cls, the lower half a whole word
        while (bits < 64 && (uint64_t(1) << (bits - 32)) < 2 * uint64_t(from.n_cls)) bits++;
        if (int rc = sort(n, bits)) return rc;
        *n_out = n;
        return VPR_OK;
    }
    // heads, ranks and ids of the n sorted pairs into `to` (from null: the base level); `level` is the length written
    int rank(size_t n, const Ids *from, int d, Ids *to, int level) {
        to->n_cls = 0;
        HIPCHK(h, hipMemsetAsync(to->F, 0xFF, size_t(n_pad) * 4, h->stream));
        HIPCHK(h, hipMemsetAsync(to->R, 0xFF, size_t(n_pad) * 4, h->stream));
        if (!n) return VPR_OK;
        if (int rc = W.seg_end()) return rc;
        if (int rc = lrep_need(h, heads, (n + 1) * 8, "class heads and their scan")) return rc;
        if (int rc = W.seg_begin()) return rc;
        uint32_t *hd = as<uint32_t>(heads), *sc = hd + (n + 1);
        const uint32_t *F = from ? from->F : nullptr, *R = from ? from->R : nullptr;
        hipLaunchKernelGGL(k_lrep_heads, dim3(blocks_of(int64_t(n) + 1)), dim3(256), 0, h->stream, keys_out, vals_out, uint64_t(n), F, R, d, hd);
        HIPCHK(h, hipGetLastError());
        if (int rc = scan(hd, sc, n + 1)) return rc;
        uint32_t n_cls = 0;
        HIPCHK(h, hipMemcpyAsync(&n_cls, sc + n, 4, hipMemcpyDeviceToHost, h->stream));
        if (int rc = W.seg_end()) return rc;
        if (n_cls >= 0x7FFFFFFFu)
            return fail(h, VPR_ERR_ARG, "%s: level %d keeps %u classes, which 31-bit ranks cannot name", ENTRY, level, n_cls);
        if (int rc = W.seg_begin()) return rc;
        hipLaunchKernelGGL(k_lrep_ids, dim3(blocks_of(int64_t(n))), dim3(256), 0, h->stream, keys_out, vals_out, uint64_t(n), sc, F, R, d, d_seq, to->F, to->R);
        HIPCHK(h, hipGetLastError());
        to->n_cls = n_cls;
        return VPR_OK;
    }
};

}  // namespace

void longrepeats_free(vpr_handle *h) {
    LongRepeatState *S = h->longrepeats;
    if (!S) return;
    (void)hipStreamSynchronize(h->stream);
    for (int k = 0; k < 2; k++) if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
    delete S;
    h->longrepeats = nullptr;
}

extern "C" {

int vpr_longrepeats_default(const vpr_repeat_stratum **spec, const char *const **names, int32_t *n) {
    if (!spec || !names || !n) return VPR_ERR_ARG;
    *spec = DEFAULT_SPEC; *names = DEFAULT_NAMES; *n = int32_t(sizeof(DEFAULT_SPEC) / sizeof(DEFAULT_SPEC[0]));
    return VPR_OK;
}

int vpr_longrepeat_intervals(vpr_handle *h, int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, const vpr_repeat_stratum *spec,
                             int32_t n_spec) {
    if (!h) return VPR_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    longrepeats_free(h);                 // the intervals of the last call end with this one, whatever becomes of it
    // every check comes before a byte of ctg_seq is read
    if (!spec) return fail(h, VPR_ERR_ARG, "%s: null spec", ENTRY);
    if (n_spec < 1 || n_spec > VPR_LREP_MAX_SPEC) return fail(h, VPR_ERR_ARG, "%s: n_spec %d is not in 1..%d", ENTRY, n_spec, VPR_LREP_MAX_SPEC);
    for (int e = 0; e < n_spec; e++) {
        if (spec[e].k < VPR_LREP_MIN_K || spec[e].k > VPR_LREP_MAX_K)
            return fail(h, VPR_ERR_ARG, "%s: entry %d: k %d is not in %d..%d", ENTRY, e, spec[e].k, VPR_LREP_MIN_K, VPR_LREP_MAX_K);
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

    LongRepeatState *S = h->longrepeats = new LongRepeatState();
    for (int k = 0; k < 2; k++) HIPCHK(h, hipEventCreate(&S->ev[k]));
    S->n_spec = n_spec; S->n_ctg = n_ctg;
    S->n_valid.assign(size_t(n_spec), 0); S->n_repeated.assign(size_t(n_spec), 0); S->n_last.assign(size_t(n_spec), 0);
    const size_t rows = size_t(n_spec) * size_t(n_ctg);

    // the entries in the order of their k (ties in the caller's order): slot s of the device tables is entry order[s]
    std::vector<int> order(size_t(n_spec), 0);
    for (int e = 0; e < n_spec; e++) order[size_t(e)] = e;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return spec[x].k < spec[y].k; });

    DevBuf<int64_t> d_off;               // [rows + 1] in slot order; the intervals behind them
    DevBuf<int32_t> d_start, d_stop;
    struct Rows {                        // (released on every way out)
        vpr_handle *h; DevBuf<int64_t> &o; DevBuf<int32_t> &a, &b;
        ~Rows() { (void)hipStreamSynchronize(h->stream); dev_release(h, o, a, b); }
    } rows_guard{h, d_off, d_start, d_stop};
    if (int rc = ctx_need(h, ENTRY, d_off, 8 * (rows + 1), "row offsets")) return rc;
    if (int rc = ctx_need(h, ENTRY, d_start, 4 * 1024, "intervals")) return rc;
    if (int rc = ctx_need(h, ENTRY, d_stop, 4 * 1024, "intervals")) return rc;

    CtxWork W(h, ENTRY);
    LongWork L(h, W);
    // the sequence, padded with zero bytes (not called) to whole tiles plus one, so that every 16-byte load of the pack stays inside
    const int64_t n_tiles_all = (N + REP_PACK_TILE - 1) / REP_PACK_TILE, n_pad = n_tiles_all * REP_PACK_TILE + REP_PACK_TILE;
    const int64_t nw_all = n_tiles_all * (REP_PACK_TILE / 64);              // 64-bit flag words of the genome
    const int64_t n_tiles_pairs = (N + LR_TILE - 1) / LR_TILE;
    if (int rc = lrep_need(h, W.seq, size_t(n_pad), "contig sequences")) return rc;
    if (int rc = W.need(W.ctg_off, 8 * (size_t(n_ctg) + 1), "contig offsets")) return rc;
    if (int rc = W.need(W.small, 256, "counters")) return rc;
    if (int rc = lrep_need(h, L.flags, size_t(nw_all) * 8 + 8, "flag bits")) return rc;
    if (int rc = W.need(L.cnt, size_t(std::max(n_tiles_all, n_tiles_pairs) + 1) * 8, "workgroup counts")) return rc;
    if (int rc = lrep_need(h, L.ids, size_t(n_pad) * 16, "id arrays, two levels")) return rc;
    if (N) HIPCHK(h, hipMemcpyAsync(W.seq.p, ctg_seq, size_t(N), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(as<uint8_t>(W.seq) + N, 0, size_t(n_pad - N), h->stream));
    HIPCHK(h, hipMemcpyAsync(W.ctg_off.p, ctg_off, 8 * (size_t(n_ctg) + 1), hipMemcpyHostToDevice, h->stream));
    L.d_seq = as<uint8_t>(W.seq); L.d_ctg = as<int64_t>(W.ctg_off); L.n_ctg = n_ctg; L.N = N; L.n_pad = n_pad;
    L.d_count = reinterpret_cast<unsigned long long *>(as<uint8_t>(W.small) + 128);   // (the run passes use the first word)

    // pieces of whole contigs for the run passes, as in vpr_repeat_intervals
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

    // the base level: the pack at k = 32, the sort over all 64 key bits, ranks and ids into slot 0
    Ids cur = L.slot(0), nxt = L.slot(1);
    int cur_len = LR_BASE;
    {
        W.ms = &S->ms_base;
        uint32_t n = 0;
        uint32_t *cnt = as<uint32_t>(L.cnt), *off = cnt + (n_tiles_all + 1);
        if (int rc = W.seg_begin()) return rc;
        if (n_tiles_all) {
            HIPCHK(h, hipMemsetAsync(cnt + n_tiles_all, 0, 4, h->stream));
            rep_launch_pack(h->stream, false, unsigned(n_tiles_all), L.d_seq, L.d_ctg, n_ctg, N, LR_BASE, cnt, nullptr, nullptr);
            HIPCHK(h, hipGetLastError());
            if (int rc = L.scan(cnt, off, size_t(n_tiles_all + 1))) return rc;
            HIPCHK(h, hipMemcpyAsync(&n, off + n_tiles_all, 4, hipMemcpyDeviceToHost, h->stream));
        }
        if (int rc = W.seg_end()) return rc;
        S->n_level[0] = int64_t(n);
        if (n) if (int rc = L.pair_room(n)) return rc;
        if (int rc = W.seg_begin()) return rc;
        if (n) {
            rep_launch_pack(h->stream, true, unsigned(n_tiles_all), L.d_seq, L.d_ctg, n_ctg, N, LR_BASE, off, as<uint64_t>(L.keys), as<uint32_t>(L.vals));
            HIPCHK(h, hipGetLastError());
            if (int rc = L.sort(n, 64)) return rc;
        }
        if (int rc = L.rank(n, nullptr, 0, &cur, LR_BASE)) return rc;
        if (W.open) if (int rc = W.seg_end()) return rc;
    }

    int64_t n_iv = 0;
    for (int s = 0; s < n_spec; s++) {
        const int e = order[size_t(s)], k = spec[e].k;
        // the doubling levels this entry needs and the call does not have yet: 64 for k > 64, 128 for k > 128
        while (2 * cur_len < k) {
            W.ms = &S->ms_levels;
            uint32_t n = 0;
            if (int rc = W.seg_begin()) return rc;
            if (int rc = L.pairs(cur, cur_len, cur_len, &n)) return rc;
            S->n_level[cur_len == LR_BASE ? 1 : 2] = int64_t(n);
            if (int rc = L.rank(n, &cur, cur_len, &nxt, 2 * cur_len)) return rc;
            if (W.open) if (int rc = W.seg_end()) return rc;
            std::swap(cur, nxt);
            cur_len *= 2;
        }
        // the last level: valid starts, pairs, sort, mark
        W.ms = &S->ms_last;
        unsigned long long n_valid = 0, n_rep = 0;
        uint32_t n = 0;
        if (int rc = W.seg_begin()) return rc;
        HIPCHK(h, hipMemsetAsync(L.d_count, 0, 16, h->stream));
        if (N) {
            hipLaunchKernelGGL(k_lrep_valid, dim3(blocks_of((N + LR_ENDS - 1) / LR_ENDS)), dim3(256), 0, h->stream, L.d_seq, L.d_ctg, n_ctg, N, k, L.d_count);
            HIPCHK(h, hipGetLastError());
        }
        if (int rc = L.pairs(cur, cur_len, k - cur_len, &n)) return rc;
        HIPCHK(h, hipMemsetAsync(L.flags.p, 0, size_t(nw_all) * 8 + 8, h->stream));
        if (n) {
            rep_launch_mark(h->stream, L.keys_out, L.vals_out, uint64_t(n), k, as<uint32_t>(L.flags), L.d_count + 1);
            HIPCHK(h, hipGetLastError());
        }
        HIPCHK(h, hipMemcpyAsync(&n_valid, L.d_count, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&n_rep, L.d_count + 1, 8, hipMemcpyDeviceToHost, h->stream));
        if (int rc = W.seg_end()) return rc;
        S->n_valid[size_t(e)] = int64_t(n_valid); S->n_repeated[size_t(e)] = int64_t(n_rep); S->n_last[size_t(e)] = int64_t(n);

        W.ms = &S->ms_intervals;
        int64_t *row_off = d_off.p + size_t(s) * size_t(n_ctg);
        const CtxRunRule rule = {k - 1, 1, 0, spec[e].slop, 1, false};
        for (const Piece &pc : pieces) {
            const int64_t g0 = ctg_off[pc.c0], g1 = ctg_off[pc.c1], T0 = g0 / REP_PACK_TILE * REP_PACK_TILE;
            const int64_t n_tiles = (g1 - T0 + REP_PACK_TILE - 1) / REP_PACK_TILE, nw = n_tiles * (REP_PACK_TILE / 64);
            uint32_t n_out = 0;
            if (int rc = W.seg_begin()) return rc;
            if (nw) {
                if (int rc = W.need(W.bits, size_t(nw) * 8, "flag bits of a piece")) return rc;
                rep_launch_piece_words(h->stream, as<uint64_t>(L.flags), nw, T0, g0, g1, as<uint64_t>(W.bits));
                HIPCHK(h, hipGetLastError());
            }
            if (int rc = ctx_intervals_from_flags(W, as<uint64_t>(W.bits), nw, T0, g0, L.d_seq, L.d_ctg, n_ctg, pc.c0, pc.c1, rule, e, d_start, d_stop,
                                                  size_t(n_iv), row_off, &n_out))
                return rc;
            n_iv += n_out;
        }
        if (W.open) if (int rc = W.seg_end()) return rc;
    }

    // the rows back in the caller's order, on the host (they are what the entries below hand out)
    std::vector<int64_t> off_s(rows + 1, 0);
    std::vector<int32_t> st_s(size_t(n_iv), 0), sp_s(size_t(n_iv), 0);
    HIPCHK(h, hipMemcpyAsync(off_s.data(), d_off.p, 8 * (rows + 1), hipMemcpyDeviceToHost, h->stream));
    if (n_iv) {
        HIPCHK(h, hipMemcpyAsync(st_s.data(), d_start.p, 4 * size_t(n_iv), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(sp_s.data(), d_stop.p, 4 * size_t(n_iv), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    off_s[rows] = n_iv;
    std::vector<int> slot_of(size_t(n_spec), 0);
    for (int s = 0; s < n_spec; s++) slot_of[size_t(order[size_t(s)])] = s;
    S->off.assign(rows + 1, 0);
    S->start.clear(); S->stop.clear();
    S->start.reserve(size_t(n_iv)); S->stop.reserve(size_t(n_iv));
    for (int e = 0; e < n_spec; e++)
        for (int c = 0; c < n_ctg; c++) {
            const size_t r = size_t(slot_of[size_t(e)]) * size_t(n_ctg) + size_t(c);
            S->off[size_t(e) * size_t(n_ctg) + size_t(c)] = int64_t(S->start.size());
            S->start.insert(S->start.end(), st_s.begin() + off_s[r], st_s.begin() + off_s[r + 1]);
            S->stop.insert(S->stop.end(), sp_s.begin() + off_s[r], sp_s.begin() + off_s[r + 1]);
        }
    S->off[rows] = int64_t(S->start.size());
    S->valid = true;
    return VPR_OK;
}

int vpr_longrepeat_interval_counts(vpr_handle *h, int64_t *iv_off) {
    if (!h || !iv_off) return VPR_ERR_ARG;
    const LongRepeatState *S = h->longrepeats;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_longrepeat_interval_counts before vpr_longrepeat_intervals");
    std::copy(S->off.begin(), S->off.end(), iv_off);
    return VPR_OK;
}

int vpr_longrepeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop) {
    if (!h) return VPR_ERR_ARG;
    const LongRepeatState *S = h->longrepeats;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_longrepeat_download_intervals before vpr_longrepeat_intervals");
    if (S->start.empty()) return VPR_OK;
    if (!start || !stop) return fail(h, VPR_ERR_ARG, "vpr_longrepeat_download_intervals: null buffer");
    std::copy(S->start.begin(), S->start.end(), start);
    std::copy(S->stop.begin(), S->stop.end(), stop);
    return VPR_OK;
}

int vpr_longrepeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated, int64_t *n_last, int64_t *n_level) {
    if (!h) return VPR_ERR_ARG;
    const LongRepeatState *S = h->longrepeats;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_longrepeat_stats before vpr_longrepeat_intervals");
    if (!n_valid || !n_repeated || !n_last) return fail(h, VPR_ERR_ARG, "vpr_longrepeat_stats: null buffer");
    for (int e = 0; e < S->n_spec; e++) {
        n_valid[e] = S->n_valid[size_t(e)]; n_repeated[e] = S->n_repeated[size_t(e)]; n_last[e] = S->n_last[size_t(e)];
    }
    if (n_level) for (int k = 0; k < 3; k++) n_level[k] = S->n_level[k];
    return VPR_OK;
}

int vpr_longrepeat_timing(const vpr_handle *h, double *ms_base, double *ms_levels, double *ms_last, double *ms_intervals) {
    if (!h || !ms_base || !ms_levels || !ms_last || !ms_intervals) return VPR_ERR_ARG;
    const LongRepeatState *S = h->longrepeats;
    if (!S || !S->valid) { *ms_base = *ms_levels = *ms_last = *ms_intervals = 0; return VPR_OK; }
    *ms_base = S->ms_base; *ms_levels = S->ms_levels; *ms_last = S->ms_last; *ms_intervals = S->ms_intervals;
    return VPR_OK;
}

}  // extern "C"
