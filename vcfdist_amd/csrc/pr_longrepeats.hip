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
// The upload, the compaction, the sort, the mark and the rows are KmerWork's (pr_kmer.h, defined in pr_repeats.hip); LongWork
// below adds the id arrays and the levels.  Device memory: the formula of pr_kmer.h, the pairs being the valid 32-mer starts (the
// upper levels use the same buffers for their candidates only), + 16 N (four id arrays: F and R of the level read and of the level
// written) + 8 bytes per valid 32-mer start (class heads and their scan).  The buckets KmerState::ms[0..3] are base, levels,
// last, intervals.
#include "pr_kmer.h"
#include "pr_plan.h"
#include "pr_ctxdev.h"
#include "../../include/vcfdist_longrepeats.h"

struct LongRepeatState : KmerState {
    std::vector<int64_t> n_last;                       // [n_spec]
    int64_t n_level[3] = {0, 0, 0};                    // pairs sorted by the base level, the level 64 and the level 128
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

struct Ids { uint32_t *F, *R; uint32_t n_cls; };       // a level's id arrays and the kept classes they name

// What the long family has beside KmerWork's arrays (released when the call goes): the id arrays, the class heads, the levels.
struct LongWork {
    vpr_handle *h;
    KmerWork &K;
    CtxWork &W;
    DevBuf<uint8_t> heads, ids;
    LongWork(vpr_handle *h_, KmerWork &K_) : h(h_), K(K_), W(K_.W) {}
    ~LongWork() {
        (void)hipStreamSynchronize(h->stream);
        dev_release(h, heads, ids);
    }
    Ids slot(int s) const { return {as<uint32_t>(ids) + size_t(2 * s) * size_t(K.n_pad), as<uint32_t>(ids) + size_t(2 * s + 1) * size_t(K.n_pad), 0}; }

    // the candidates of the level from -> from + d, sorted; *n_out of them.  A timed segment is under way on entry and on return.
    int pairs(const Ids &from, int a, int d, uint32_t *n_out) {
        *n_out = 0;
        if (!from.n_cls) return VPR_OK;  // (nothing is kept: no start has two kept halves)
        const int64_t n_tiles = (K.N + LR_TILE - 1) / LR_TILE;
        uint32_t n = 0;
        const auto launch = [&](bool write, uint32_t *out, uint64_t *ks, uint32_t *vs) {
            const auto kernel = write ? k_lrep_pairs<true> : k_lrep_pairs<false>;
            hipLaunchKernelGGL(kernel, dim3(unsigned(n_tiles)), dim3(256), 0, h->stream, from.F, from.R, K.d_ctg, K.n_ctg, K.N, d, int(d == a), out, ks, vs);
        };
        if (int rc = K.compact(n_tiles, launch, &n)) return rc;
        if (!n) return VPR_OK;
        unsigned bits = 33;              // the upper half is an id below 2 n_cls, the lower half a whole word
        while (bits < 64 && (uint64_t(1) << (bits - 32)) < 2 * uint64_t(from.n_cls)) bits++;
        if (int rc = K.sort(n, bits)) return rc;
        *n_out = n;
        return VPR_OK;
    }
    // heads, ranks and ids of the n sorted pairs into `to` (from null: the base level); `level` is the length written
    int rank(size_t n, const Ids *from, int d, Ids *to, int level) {
        to->n_cls = 0;
        HIPCHK(h, hipMemsetAsync(to->F, 0xFF, size_t(K.n_pad) * 4, h->stream));
        HIPCHK(h, hipMemsetAsync(to->R, 0xFF, size_t(K.n_pad) * 4, h->stream));
        if (!n) return VPR_OK;
        if (int rc = W.seg_end()) return rc;
        if (int rc = K.need(heads, (n + 1) * 8, "class heads and their scan")) return rc;
        if (int rc = W.seg_begin()) return rc;
        uint32_t *hd = as<uint32_t>(heads), *sc = hd + (n + 1);
        const uint32_t *F = from ? from->F : nullptr, *R = from ? from->R : nullptr;
        hipLaunchKernelGGL(k_lrep_heads, dim3(blocks_of(int64_t(n) + 1)), dim3(256), 0, h->stream, K.keys_out, K.vals_out, uint64_t(n), F, R, d, hd);
        HIPCHK(h, hipGetLastError());
        if (int rc = K.scan(hd, sc, n + 1)) return rc;
        uint32_t n_cls = 0;
        HIPCHK(h, hipMemcpyAsync(&n_cls, sc + n, 4, hipMemcpyDeviceToHost, h->stream));
        if (int rc = W.seg_end()) return rc;
        if (n_cls >= 0x7FFFFFFFu)
            return fail(h, VPR_ERR_ARG, "%s: level %d keeps %u classes, which 31-bit ranks cannot name", ENTRY, level, n_cls);
        if (int rc = W.seg_begin()) return rc;
        hipLaunchKernelGGL(k_lrep_ids, dim3(blocks_of(int64_t(n))), dim3(256), 0, h->stream, K.keys_out, K.vals_out, uint64_t(n), sc, F, R, d, K.d_seq, to->F, to->R);
        HIPCHK(h, hipGetLastError());
        to->n_cls = n_cls;
        return VPR_OK;
    }
};

}  // namespace

void longrepeats_free(vpr_handle *h) { kmer_free(h, &vpr_handle::longrepeats); }

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
    if (int rc = KmerWork::check_args(h, ENTRY, VPR_LREP_MIN_K, VPR_LREP_MAX_K, VPR_LREP_MAX_SPEC, n_ctg, ctg_off, ctg_seq, spec, n_spec)) return rc;
    LongRepeatState *S = h->longrepeats = new LongRepeatState();
    if (int rc = S->init(h, n_spec, n_ctg)) return rc;
    S->n_last.assign(size_t(n_spec), 0);
    const size_t rows = size_t(n_spec) * size_t(n_ctg);

    // the entries in the order of their k (ties in the caller's order): slot s of the device tables is entry order[s]
    std::vector<int> order(size_t(n_spec), 0);
    for (int e = 0; e < n_spec; e++) order[size_t(e)] = e;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return spec[x].k < spec[y].k; });

    KmerWork K(h, ENTRY);
    LongWork L(h, K);
    CtxWork &W = K.W;
    if (int rc = K.upload(n_ctg, ctg_off, ctg_seq, rows, LR_TILE)) return rc;
    if (int rc = K.need(L.ids, size_t(K.n_pad) * 16, "id arrays, two levels")) return rc;
    if (int rc = K.begin_timing(S)) return rc;           // (behind the last allocation: a large one leaves work on the device)
    const int64_t N = K.N;

    // the base level: the pack at k = 32, the sort over all 64 key bits, ranks and ids into slot 0
    Ids cur = L.slot(0), nxt = L.slot(1);
    int cur_len = LR_BASE;
    {
        W.ms = &S->ms[0];
        uint32_t n = 0;
        if (int rc = W.seg_begin()) return rc;
        if (int rc = K.pack(LR_BASE, &n)) return rc;
        S->n_level[0] = int64_t(n);
        if (n) if (int rc = K.sort(n, 64)) return rc;
        if (int rc = L.rank(n, nullptr, 0, &cur, LR_BASE)) return rc;
        if (W.open) if (int rc = W.seg_end()) return rc;
    }

    int64_t n_iv = 0;
    for (int s = 0; s < n_spec; s++) {
        const int e = order[size_t(s)], k = spec[e].k;
        // the doubling levels this entry needs and the call does not have yet: 64 for k > 64, 128 for k > 128
        while (2 * cur_len < k) {
            W.ms = &S->ms[1];
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
        W.ms = &S->ms[2];
        unsigned long long n_valid = 0, n_rep = 0;
        uint32_t n = 0;
        if (int rc = W.seg_begin()) return rc;
        HIPCHK(h, hipMemsetAsync(K.d_count, 0, 8, h->stream));
        if (N) {
            hipLaunchKernelGGL(k_lrep_valid, dim3(blocks_of((N + LR_ENDS - 1) / LR_ENDS)), dim3(256), 0, h->stream, K.d_seq, K.d_ctg, n_ctg, N, k, K.d_count);
            HIPCHK(h, hipGetLastError());
        }
        if (int rc = L.pairs(cur, cur_len, k - cur_len, &n)) return rc;
        if (int rc = K.mark(n, k, &n_rep)) return rc;
        HIPCHK(h, hipMemcpyAsync(&n_valid, K.d_count, 8, hipMemcpyDeviceToHost, h->stream));
        if (int rc = W.seg_end()) return rc;
        S->n_valid[size_t(e)] = int64_t(n_valid); S->n_repeated[size_t(e)] = int64_t(n_rep); S->n_last[size_t(e)] = int64_t(n);

        W.ms = &S->ms[3];
        if (int rc = K.rows_of_entry(k, spec[e].slop, e, s, &n_iv)) return rc;
    }

    // the rows back in the caller's order, on the host
    std::vector<int64_t> off_s;
    std::vector<int32_t> st_s, sp_s;
    if (int rc = K.download_rows(n_iv, off_s, st_s, sp_s)) return rc;
    std::vector<int> slot_of(size_t(n_spec), 0);
    for (int s = 0; s < n_spec; s++) slot_of[size_t(order[size_t(s)])] = s;
    S->off.assign(rows + 1, 0);
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
    return h ? kmer_interval_counts(h, h->longrepeats, "vpr_longrepeat_interval_counts", ENTRY, iv_off) : VPR_ERR_ARG;
}

int vpr_longrepeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop) {
    return h ? kmer_download_intervals(h, h->longrepeats, "vpr_longrepeat_download_intervals", ENTRY, start, stop) : VPR_ERR_ARG;
}

int vpr_longrepeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_repeated, int64_t *n_last, int64_t *n_level) {
    if (!h) return VPR_ERR_ARG;
    const LongRepeatState *S = h->longrepeats;
    if (int rc = kmer_stats(h, S, "vpr_longrepeat_stats", ENTRY, n_last != nullptr, n_valid, n_repeated)) return rc;
    std::copy(S->n_last.begin(), S->n_last.end(), n_last);
    if (n_level) for (int k = 0; k < 3; k++) n_level[k] = S->n_level[k];
    return VPR_OK;
}

int vpr_longrepeat_timing(const vpr_handle *h, double *ms_base, double *ms_levels, double *ms_last, double *ms_intervals) {
    return h ? kmer_timing(h->longrepeats, ms_base, ms_levels, ms_last, ms_intervals) : VPR_ERR_ARG;
}

}  // extern "C"
