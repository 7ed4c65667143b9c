// pr_context.hip -- the sequence-context strata (include/vcfdist_context.h): sorted interval lists per (stratum, contig) built on
// the device from the contig sequences, and handed to k_strata_mask (pr_strata.hip) without leaving it.
//
// Both predicates of the header are local, so nothing is carried between tiles.  Per stratum and piece of the genome:
//   1. k_ctx_flags_period<P> / k_ctx_flags_gc   one flag bit per base (16-byte loads with a halo of P resp. W bases; GC windows are
//                                               differences of running counts kept in LDS, never summed one by one)
//   2. k_ctx_run_count                          run starts (m[i] && !m[i-1]) and run ends (m[i] && !m[i+1]) per workgroup; runs too
//                                               short for a period stratum's min_len are dropped here where that fits a flag word
//   3. exclusive scans of the workgroup counts  (rocPRIM, pr_plan.hip)
//   4. k_ctx_run_write                          starts and ends in position order (the k-th start belongs to the k-th end)
//   5. k_ctx_keep, a scan, k_ctx_compact        length and primitive test per tract (O(p)), then pad and clip
//   6. k_ctx_group, a scan, k_ctx_merge         kept tracts have increasing starts and stops, so "starts a new merged interval"
//                                               is a comparison with the previous kept tract alone
//   7. k_ctx_rows                               the rows' offsets (one bisection per contig)
// Passes 2 to 7 are ctx_intervals_from_flags (pr_host.h), which pr_repeats.hip calls with flag bits of its own.
// No pass compacts with atomics: every output index is a prefix sum, so two calls give identical arrays.  No pass walks a
// run: a 100 kb homopolymer is 100 k flag bits and one start / end pair.
//
// Workspace: 1/8 byte per base (the flag bits) + 16 bytes per 16 384 bases (workgroup counts and their scans), and 28 bytes
// per run the run passes emit (start, end, keep / group flag, its scan, and contig, padded start, padded stop of the kept ones).
// The genome is taken in pieces of whole contigs of at most PIECE_BASES bases (a longer contig is a piece of its own: a contig
// is not split), which bounds the per-base part; the sequence itself (one byte per base) is resident for the call.
#include "pr_host.h"
#include "pr_plan.h"
#include "pr_ctxdev.h"
#include "../../include/vcfdist_context.h"

struct ContextState {
    int32_t n_spec = 0, n_ctg = 0, n_bed = 0;
    int64_t n_iv_bed = 0, n_iv_ctx = 0;
    // one table for the mask kernel: the rows of the BED strata first, the context rows behind them
    DevBuf<int64_t> d_off;                             // [(n_bed + n_spec) * n_ctg + 1]
    DevBuf<int32_t> d_start, d_stop;                   // [n_iv_bed + n_iv_ctx]
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_intervals = 0, ms_mask = 0;
    bool valid = false;
};

namespace {

const int CTX_LANE = 16, CTX_WG = 256, CTX_TILE = CTX_LANE * CTX_WG;      // the flag kernels: bases of a lane / a workgroup
const int RUN_TILE = 64 * 256;                                            // the run kernels: a 64-bit flag word per lane
static_assert(RUN_TILE % CTX_TILE == 0, "the run kernels' seams are seams of the flag kernels");
const int64_t PIECE_BASES = int64_t(1) << 28;
const int GC_LDS_MAX_W = 8192;         // windows up to this take their counts from a table in LDS (4 bytes per byte of tile and halo: 48 KiB)

const vpr_context_stratum DEFAULT_SPEC[] = {
    {VPR_CTX_PERIOD, 1, 4, 6, 0, 0, 0, 5},  {VPR_CTX_PERIOD, 1, 7, 11, 0, 0, 0, 5}, {VPR_CTX_PERIOD, 1, 12, 0, 0, 0, 0, 5},
    {VPR_CTX_PERIOD, 2, 10, 0, 0, 0, 0, 5}, {VPR_CTX_PERIOD, 3, 14, 0, 0, 0, 0, 5}, {VPR_CTX_PERIOD, 4, 19, 0, 0, 0, 0, 5},
    {VPR_CTX_GC, 0, 0, 0, 0, 25, 100, 0},   {VPR_CTX_GC, 0, 0, 0, 25, 30, 100, 0},  {VPR_CTX_GC, 0, 0, 0, 30, 55, 100, 0},
    {VPR_CTX_GC, 0, 0, 0, 55, 65, 100, 0},  {VPR_CTX_GC, 0, 0, 0, 65, 101, 100, 0},
};
const char *const DEFAULT_NAMES[] = {"hp_4to6", "hp_7to11", "hp_ge12", "tr_di_ge10", "tr_tri_ge14", "tr_quad_ge19",
                                     "gc_lt25", "gc_25to30", "gc_30to55", "gc_55to65", "gc_ge65"};

// 0x01 in every byte of x that equals the byte repeated in c4
__device__ inline uint32_t eq_bytes(uint32_t x, uint32_t c4) {
    const uint32_t t = x ^ c4;
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu) >> 7;
}

}  // namespace

// Flag bits of a period stratum: lane t takes the 16 bases from T0 + 16 t (its 16-byte load, and the 16 bytes in front of
// them for s[i - P]) and stores 16 bits.  Bases outside the piece [g0, g1) and the first P bases of every contig get 0, so no
// run of flags crosses a contig start.
template <int P>
__global__ void __launch_bounds__(256) k_ctx_flags_period(const uint8_t *__restrict__ seq, const int64_t *__restrict__ ctg_off, int n_ctg,
                                                          int64_t T0, int64_t g0, int64_t g1, uint16_t *__restrict__ bits) {
    const int64_t t = int64_t(blockIdx.x) * CTX_WG + threadIdx.x, G = T0 + t * CTX_LANE;
    unsigned f = 0;
    if (G + CTX_LANE > g0 && G < g1) {
        const uint4 cur = *reinterpret_cast<const uint4 *>(seq + G);
        const uint4 prv = G >= 16 ? *reinterpret_cast<const uint4 *>(seq + G - 16) : make_uint4(0, 0, 0, 0);
        const uint32_t w[8] = {prv.x, prv.y, prv.z, prv.w, cur.x, cur.y, cur.z, cur.w};
        int c = ctg_of(ctg_off, n_ctg, G > g0 ? G : g0);
        int64_t cs = ctg_off[c], ce = ctg_off[c + 1];
        if (G >= g0 && G + CTX_LANE <= g1 && G - cs >= P && G + CTX_LANE <= ce) {
            // the whole stretch inside the piece and one contig, P bases in: four bases at a time, no test per base
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x = w[4 + k];
                const uint32_t y = P <= 4 ? uint32_t((uint64_t(w[4 + k]) << 32 | w[3 + k]) >> (8 * (4 - P)))
                                          : uint32_t((uint64_t(w[3 + k]) << 32 | w[2 + k]) >> (8 * (8 - P)));
                const uint32_t ok = eq_bytes(x ^ y, 0u) & (eq_bytes(x, 0x41414141u) | eq_bytes(x, 0x43434343u) | eq_bytes(x, 0x47474747u) |
                                                           eq_bytes(x, 0x54545454u));
                f |= ((ok * 0x01020408u) >> 24 & 15u) << (4 * k);       // the four 0x01 bytes as four bits
            }
        } else
#pragma unroll
        for (int j = 0; j < CTX_LANE; j++) {
            const int64_t Gj = G + j;
            if (Gj < g0 || Gj >= g1) continue;
            while (Gj >= ce) { c++; cs = ctg_off[c]; ce = ctg_off[c + 1]; }      // (ends: Gj < g1 <= ctg_off[n_ctg])
            const unsigned x = (w[(16 + j) >> 2] >> (((16 + j) & 3) * 8)) & 255u;
            const unsigned y = (w[(16 + j - P) >> 2] >> (((16 + j - P) & 3) * 8)) & 255u;
            if (Gj - cs >= P && x == y && called(x)) f |= 1u << j;
        }
    }
    bits[t] = uint16_t(f);
}

extern "C" {

// Flag bits of a GC stratum.  Phase 1: the workgroup reads the bytes its windows touch (tile plus a halo of W) with 16-byte
// loads, classes four bases at a time (G/C, uncalled) and leaves their running counts in LDS: pre[b] = (uncalled << 16 | G/C)
// among the bytes [A, A + b).  Phase 2: a window's two counts are one subtraction of two LDS words, so a window never gets
// summed at all; a wave takes 64 consecutive bases at a time (conflict-free reads) and its ballot is the flag word.  Bytes
// outside the concatenation read as 0 (not called); a window that leaves its contig is refused by the bounds test.
__global__ void __launch_bounds__(256) k_ctx_flags_gc(const uint8_t *__restrict__ seq, int64_t n_pad, const int64_t *__restrict__ ctg_off,
                                                      int n_ctg, int64_t T0, int64_t g0, int64_t g1, int W, int lo, int hi,
                                                      uint64_t *__restrict__ words) {
    extern __shared__ uint4 pre4[];
    __shared__ uint32_t part[4];
    uint32_t *pre = reinterpret_cast<uint32_t *>(pre4);
    const int half = W / 2;
    const int64_t tile = T0 + int64_t(blockIdx.x) * CTX_TILE;
    const int64_t A = (tile - half) & ~int64_t(15), E = (tile + CTX_TILE + (W - half) + 15) & ~int64_t(15);
    const int n16 = int((E - A) >> 4);
    uint32_t carry = 0;
    for (int k0 = 0; k0 < n16; k0 += CTX_WG) {
        const int k = k0 + threadIdx.x;
        const int64_t Gk = A + int64_t(k) * 16;
        const uint4 q = (k < n16 && Gk >= 0 && Gk < n_pad) ? *reinterpret_cast<const uint4 *>(seq + Gk) : make_uint4(0, 0, 0, 0);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        uint32_t inc[16], run = 0;                   // counts among the chunk's bytes [0, m], packed as in pre[]
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t gc = eq_bytes(w[i], 0x47474747u) | eq_bytes(w[i], 0x43434343u);
            const uint32_t bad = (gc | eq_bytes(w[i], 0x41414141u) | eq_bytes(w[i], 0x54545454u)) ^ 0x01010101u;
            const uint32_t gp = gc * 0x01010101u, bp = bad * 0x01010101u;      // byte m: the count among bytes 0..m of the word
#pragma unroll
            for (int m = 0; m < 4; m++) inc[4 * i + m] = run + (((bp >> (8 * m)) & 255u) << 16 | ((gp >> (8 * m)) & 255u));
            run = inc[4 * i + 3];
        }
        uint32_t total;
        const uint32_t base = carry + block_scan(k < n16 ? run : 0u, part, &total);
        if (k < n16) {
#pragma unroll
            for (int i = 0; i < 4; i++)
                pre4[4 * k + i] = make_uint4(base + (i ? inc[4 * i - 1] : 0u), base + inc[4 * i], base + inc[4 * i + 1], base + inc[4 * i + 2]);
            if (k == n16 - 1) pre[16 * n16] = base + run;
        }
        carry += total;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t lw = int64_t(lo) * W, hw = int64_t(hi) * W;
    bool have = false;
    int c = 0;
    int64_t cs = 0, ce = 0;
    if (tile >= g0 && tile + CTX_TILE <= g1) {       // (uniform) every window of the tile inside the piece and one contig: no test per base
        c = ctg_of(ctg_off, n_ctg, tile); cs = ctg_off[c]; ce = ctg_off[c + 1];
        if (tile - half >= cs && tile + CTX_TILE - 1 - half + W <= ce) {
            const int at = int(tile - half - A) + lane;
            const uint32_t lw32 = uint32_t(lw), hw32 = uint32_t(hw);          // (hi * W <= 101 * GC_LDS_MAX_W)
#pragma unroll 4
            for (int j = 0; j < 16; j++) {
                const int word = wave * 16 + j;
                const uint32_t d = pre[at + 64 * word + W] - pre[at + 64 * word], g100 = 100u * (d & 0xFFFFu);
                const uint64_t m = __ballot((d >> 16) == 0 && lw32 <= g100 && g100 < hw32);
                if (lane == 0) words[int64_t(blockIdx.x) * 64 + word] = m;
            }
            return;
        }
    }
    for (int j = 0; j < 16; j++) {
        const int word = wave * 16 + j;
        const int64_t Gi = tile + 64 * word + lane, a = Gi - half;
        bool flag = false;
        if (Gi >= g0 && Gi < g1) {
            if (!have) { c = ctg_of(ctg_off, n_ctg, Gi); cs = ctg_off[c]; ce = ctg_off[c + 1]; have = true; }
            while (Gi >= ce) { c++; cs = ctg_off[c]; ce = ctg_off[c + 1]; }      // (ends: Gi < g1 <= ctg_off[n_ctg])
            if (a >= cs && a + W <= ce) {
                const uint32_t d = pre[a + W - A] - pre[a - A];
                const int64_t g100 = int64_t(100) * (d & 0xFFFFu);
                flag = (d >> 16) == 0 && lw <= g100 && g100 < hw;
            }
        }
        const uint64_t m = __ballot(flag);
        if (lane == 0) words[int64_t(blockIdx.x) * 64 + word] = m;
    }
}

// The same for windows too wide for the LDS table: a lane sums its first window from global memory and slides it along its 16
// bases.
__global__ void __launch_bounds__(256) k_ctx_flags_gc_wide(const uint8_t *__restrict__ seq, int64_t n_pad, const int64_t *__restrict__ ctg_off,
                                                           int n_ctg, int64_t T0, int64_t g0, int64_t g1, int W, int lo, int hi,
                                                           uint16_t *__restrict__ bits) {
    const int half = W / 2;
    auto byte = [&](int64_t Gx) -> unsigned { return (Gx >= 0 && Gx < n_pad) ? seq[Gx] : 0u; };
    const int64_t t = int64_t(blockIdx.x) * CTX_WG + threadIdx.x, G = T0 + t * CTX_LANE;
    unsigned f = 0;
    if (G + CTX_LANE > g0 && G < g1) {
        int c = ctg_of(ctg_off, n_ctg, G > g0 ? G : g0);
        int64_t cs = ctg_off[c], ce = ctg_off[c + 1];
        int g = 0, bad = 0;                                           // G/C bases and uncalled bases of the window of base G
        for (int k = 0; k < W; k++) {
            const unsigned x = byte(G - half + k);
            g += (x == 'G' || x == 'C'); bad += !called(x);
        }
        const int64_t lw = int64_t(lo) * W, hw = int64_t(hi) * W;
        for (int j = 0; j < CTX_LANE; j++) {
            const int64_t Gj = G + j, a = Gj - half;
            if (Gj >= g0 && Gj < g1) {
                while (Gj >= ce) { c++; cs = ctg_off[c]; ce = ctg_off[c + 1]; }
                const int64_t g100 = int64_t(100) * g;
                if (a >= cs && a + W <= ce && bad == 0 && lw <= g100 && g100 < hw) f |= 1u << j;
            }
            const unsigned out = byte(a), in = byte(a + W);
            g += int(in == 'G' || in == 'C') - int(out == 'G' || out == 'C');
            bad += int(!called(in)) - int(!called(out));
        }
    }
    bits[t] = uint16_t(f);
}

}  // extern "C"

namespace {

// run starts and run ends among the 64 flags of word w: the neighbour of a contig's first base is "no flag"
__device__ inline void run_masks(const uint64_t *__restrict__ words, int64_t nw, int64_t w, int64_t T0, const int64_t *__restrict__ ctg_off,
                                 int n_ctg, int64_t g0, int min_run, uint64_t *st, uint64_t *en) {
    const uint64_t f = words[w];
    *st = *en = 0;
    if (!f) return;
    const uint64_t prev_w = w > 0 ? words[w - 1] : 0, next_w = w + 1 < nw ? words[w + 1] : 0;
    const uint64_t prev = prev_w >> 63, next = next_w & 1;
    const int64_t G0 = T0 + 64 * w;
    uint64_t bm = 0, bnext = 0;          // bit j: a contig starts at G0 + j; bnext: one starts at G0 + 64
    const int c = ctg_of(ctg_off, n_ctg, G0 > g0 ? G0 : g0);
    if (ctg_off[c] >= G0) bm |= uint64_t(1) << (ctg_off[c] - G0);
    for (int c2 = c + 1; c2 < n_ctg && ctg_off[c2] <= G0 + 64; c2++) {
        const int64_t d = ctg_off[c2] - G0;
        if (d < 64) bm |= uint64_t(1) << d; else bnext = uint64_t(1) << 63;
    }
    const uint64_t pv = ((f << 1) | prev) & ~bm, nx = ((f >> 1) | (next << 63)) & ~((bm >> 1) | bnext);
    *st = f & ~pv; *en = f & ~nx;
    if (min_run > 1) {
        // Runs of fewer than min_run flags (2 <= min_run <= 64; period strata only, whose runs never touch a contig start) are
        // dropped here already: a start counts iff the min_run flags from it on are set, an end iff the min_run up to it are --
        // both hold for exactly the runs of at least min_run flags, so the k-th start still belongs to the k-th end.
        typedef unsigned __int128 u128;
        u128 up = u128(next_w) << 64 | f, dn = u128(f) << 64 | prev_w;
        int have = 1;
        while (2 * have <= min_run) { up &= up >> have; dn &= dn << have; have *= 2; }
        if (min_run > have) { up &= up >> (min_run - have); dn &= dn << (min_run - have); }
        *st &= uint64_t(up); *en &= uint64_t(dn >> 64);
    }
}

// tract r of the run lists: false when the filter drops it, else its contig and its padded, clipped interval
__device__ inline bool tract_of(int64_t r, const uint32_t *__restrict__ run_st, const uint32_t *__restrict__ run_en, int64_t T0,
                                const uint8_t *__restrict__ seq, const int64_t *__restrict__ ctg_off, int n_ctg, int p, int prim, int min_len,
                                int max_len, int slop, int *c_out, int32_t *ps, int32_t *pe) {
    const int64_t a = run_st[r], b = int64_t(run_en[r]) + 1, Ga = T0 + a;
    const int c = ctg_of(ctg_off, n_ctg, Ga);
    const int64_t cs = ctg_off[c], L = ctg_off[c + 1] - cs, ts = Ga - cs - p, len = b - a + p;
    if (len < min_len || (max_len && len > max_len)) return false;
    const uint8_t *__restrict__ s = seq + cs + ts;
    for (int q = 1; q < prim; q++) {     // (prim: p for a period stratum, 0 where the primitive test does not apply)
        if (p % q) continue;
        bool rep = true;
        for (int k = q; k < p; k++) rep = rep && s[k] == s[k - q];
        if (rep) return false;               // the first p bases repeat a word of length q | p: not primitive
    }
    const int64_t lo = ts - slop, hi = ts + len + slop;
    *c_out = c; *ps = int32_t(lo < 0 ? 0 : lo); *pe = int32_t(hi > L ? L : hi);
    return true;
}

}  // namespace

extern "C" {

__global__ void __launch_bounds__(256) k_ctx_run_count(const uint64_t *__restrict__ words, int64_t nw, int64_t T0,
                                                       const int64_t *__restrict__ ctg_off, int n_ctg, int64_t g0, int min_run,
                                                       uint32_t *__restrict__ cnt_st, uint32_t *__restrict__ cnt_en) {
    __shared__ uint32_t lds[4];
    const int64_t w = int64_t(blockIdx.x) * 256 + threadIdx.x;
    uint64_t st = 0, en = 0;
    if (w < nw) run_masks(words, nw, w, T0, ctg_off, n_ctg, g0, min_run, &st, &en);
    uint32_t tot_st, tot_en;
    (void)block_scan(uint32_t(__popcll(st)), lds, &tot_st);
    (void)block_scan(uint32_t(__popcll(en)), lds, &tot_en);
    if (threadIdx.x == 0) { cnt_st[blockIdx.x] = tot_st; cnt_en[blockIdx.x] = tot_en; }
}

// positions (relative to T0) of the run starts and of the run ends (the last flagged base), each list in position order
__global__ void __launch_bounds__(256) k_ctx_run_write(const uint64_t *__restrict__ words, int64_t nw, int64_t T0,
                                                       const int64_t *__restrict__ ctg_off, int n_ctg, int64_t g0, int min_run,
                                                       const uint32_t *__restrict__ off_st, const uint32_t *__restrict__ off_en,
                                                       uint32_t *__restrict__ run_st, uint32_t *__restrict__ run_en) {
    __shared__ uint32_t lds[4];
    const int64_t w = int64_t(blockIdx.x) * 256 + threadIdx.x;
    uint64_t st = 0, en = 0;
    if (w < nw) run_masks(words, nw, w, T0, ctg_off, n_ctg, g0, min_run, &st, &en);
    uint32_t tot;
    uint32_t at = off_st[blockIdx.x] + block_scan(uint32_t(__popcll(st)), lds, &tot);
    while (st) { run_st[at++] = uint32_t(64 * w) + uint32_t(__ffsll((long long)st) - 1); st &= st - 1; }
    at = off_en[blockIdx.x] + block_scan(uint32_t(__popcll(en)), lds, &tot);
    while (en) { run_en[at++] = uint32_t(64 * w) + uint32_t(__ffsll((long long)en) - 1); en &= en - 1; }
}

__global__ void __launch_bounds__(256) k_ctx_keep(int64_t n_run, const uint32_t *__restrict__ run_st, const uint32_t *__restrict__ run_en,
                                                  int64_t T0, const uint8_t *__restrict__ seq, const int64_t *__restrict__ ctg_off, int n_ctg,
                                                  int p, int prim, int min_len, int max_len, int slop, uint32_t *__restrict__ keep /* [n_run + 1] */) {
    const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (r > n_run) return;
    int c; int32_t ps, pe;
    keep[r] = r < n_run && tract_of(r, run_st, run_en, T0, seq, ctg_off, n_ctg, p, prim, min_len, max_len, slop, &c, &ps, &pe);
}

__global__ void __launch_bounds__(256) k_ctx_compact(int64_t n_run, const uint32_t *__restrict__ run_st, const uint32_t *__restrict__ run_en,
                                                     int64_t T0, const uint8_t *__restrict__ seq, const int64_t *__restrict__ ctg_off, int n_ctg,
                                                     int p, int prim, int min_len, int max_len, int slop, const uint32_t *__restrict__ keep,
                                                     const uint32_t *__restrict__ keep_scan, int32_t *__restrict__ k_ctg,
                                                     int32_t *__restrict__ k_ps, int32_t *__restrict__ k_pe, uint32_t *__restrict__ n_kept) {
    const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (r == 0) *n_kept = keep_scan[n_run];
    if (r >= n_run || !keep[r]) return;
    int c; int32_t ps, pe;
    (void)tract_of(r, run_st, run_en, T0, seq, ctg_off, n_ctg, p, prim, min_len, max_len, slop, &c, &ps, &pe);
    const uint32_t k = keep_scan[r];
    k_ctg[k] = c; k_ps[k] = ps; k_pe[k] = pe;
}

// flag[j] = kept tract j starts a merged interval: the first one, the first of its contig, or one that neither overlaps nor
// abuts its predecessor (flag[j] = 0 for j >= *n_kept, up to the scan's extra element n_run)
__global__ void __launch_bounds__(256) k_ctx_group(int64_t n_run, const uint32_t *__restrict__ n_kept, const int32_t *__restrict__ k_ctg,
                                                   const int32_t *__restrict__ k_ps, const int32_t *__restrict__ k_pe,
                                                   uint32_t *__restrict__ flag /* [n_run + 1] */) {
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j > n_run) return;
    flag[j] = j < int64_t(*n_kept) && (j == 0 || k_ctg[j] != k_ctg[j - 1] || k_ps[j] > k_pe[j - 1]);
}

__global__ void __launch_bounds__(256) k_ctx_merge(const uint32_t *__restrict__ n_kept, const int32_t *__restrict__ k_ctg,
                                                   const int32_t *__restrict__ k_ps, const int32_t *__restrict__ k_pe,
                                                   const uint32_t *__restrict__ flag, const uint32_t *__restrict__ flag_scan,
                                                   int32_t *__restrict__ out_ctg, int32_t *__restrict__ out_start, int32_t *__restrict__ out_stop) {
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x, nk = *n_kept;
    if (j >= nk) return;
    const uint32_t gid = flag_scan[j] + flag[j] - 1;
    if (flag[j]) { out_start[gid] = k_ps[j]; out_ctg[gid] = k_ctg[j]; }
    if (j + 1 == nk || flag[j + 1]) out_stop[gid] = k_pe[j];      // (stops increase: the last member's is the union's)
}

// rows [c0, c1] of one stratum: where contig c's intervals begin among the n_out sorted by contig (the entry of c1 is the
// end of the piece, which the next piece or stratum writes again as its beginning)
__global__ void __launch_bounds__(256) k_ctx_rows(const int32_t *__restrict__ out_ctg, int64_t n_out, int c0, int c1, int64_t base,
                                                  int64_t *__restrict__ row_off /* entry of contig 0 of the stratum */) {
    const int c = c0 + int(blockIdx.x) * 256 + threadIdx.x;
    if (c > c1) return;
    int64_t lo = 0, hi = n_out;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (out_ctg[mid] < c) lo = mid + 1; else hi = mid; }
    row_off[c] = base + lo;
}

}  // extern "C"

namespace {

int check_spec(vpr_handle *h, const vpr_context_stratum *spec, int32_t n_spec) {
    for (int k = 0; k < n_spec; k++) {
        const vpr_context_stratum &s = spec[k];
        if (s.slop < 0) return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: slop %d is negative", k, s.slop);
        if (s.kind == VPR_CTX_PERIOD) {
            if (s.period < 1 || s.period > 6) return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: period %d is not in 1..6", k, s.period);
            if (s.min_len <= s.period) return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: min_len %d is not above the period %d", k, s.min_len, s.period);
            if (s.max_len != 0 && s.max_len < s.min_len)
                return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: max_len %d is neither 0 nor at least min_len %d", k, s.max_len, s.min_len);
        } else if (s.kind == VPR_CTX_GC) {
            if (s.gc_lo < 0 || s.gc_lo >= s.gc_hi || s.gc_hi > 101)
                return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: GC range %d..%d is not 0 <= lo < hi <= 101", k, s.gc_lo, s.gc_hi);
            if (s.window < 1) return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: window %d is below 1", k, s.window);
        } else {
            return fail(h, VPR_ERR_ARG, "vpr_context_masks: entry %d: unknown kind %d", k, s.kind);
        }
    }
    return VPR_OK;
}

int scan_u32(CtxWork &W, const uint32_t *in, uint32_t *out, size_t n) {
    vpr_handle *h = W.h;
    size_t bytes = 0;
    if (vplan_exclusive_scan_u32(nullptr, &bytes, in, out, n, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: scan workspace query failed", W.entry);
    if (int rc = W.need(W.tmp, bytes + 256, "scan workspace")) return rc;
    if (vplan_exclusive_scan_u32(W.tmp.p, &bytes, in, out, n, h->stream) != 0) return fail(h, VPR_ERR_DEVICE, "%s: scan failed", W.entry);
    return VPR_OK;
}

template <int P>
void launch_period(unsigned blocks, hipStream_t st, const uint8_t *seq, const int64_t *ctg_off, int n_ctg, int64_t T0, int64_t g0, int64_t g1,
                   uint16_t *bits) {
    hipLaunchKernelGGL(k_ctx_flags_period<P>, dim3(blocks), dim3(CTX_WG), 0, st, seq, ctg_off, n_ctg, T0, g0, g1, bits);
}

}  // namespace

int64_t ctx_piece_bases() {   // (VPR_CONTEXT_PIECE_BASES: a smaller piece, so that a test's few contigs make several)
    const char *e = getenv("VPR_CONTEXT_PIECE_BASES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? int64_t(v) : PIECE_BASES;
}

std::vector<CtxPiece> ctx_pieces(const int64_t *ctg_off, int n_ctg) {   // (a longer contig is a piece of its own)
    std::vector<CtxPiece> pieces;
    const int64_t budget = ctx_piece_bases();
    for (int c = 0; c < n_ctg;) {
        int e = c + 1;
        while (e < n_ctg && ctg_off[e + 1] - ctg_off[c] <= budget) e++;
        pieces.push_back({c, e});
        c = e;
    }
    return pieces;
}

int CtxWork::seg_begin() {
    if (!open) { HIPCHK(h, hipEventRecord(ev[0], h->stream)); open = true; }
    return VPR_OK;
}
int CtxWork::seg_end() {
    HIPCHK(h, hipEventRecord(ev[1], h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    float t = 0;
    (void)hipEventElapsedTime(&t, ev[0], ev[1]);
    *ms += t; open = false;
    return VPR_OK;
}

// passes 2 to 7 of the file's header; a timed segment may be under way on entry, and one is on return
int ctx_intervals_from_flags(CtxWork &W, const uint64_t *words, int64_t nw, int64_t T0, int64_t g0, const uint8_t *d_seq, const int64_t *d_ctg,
                             int n_ctg, int c0, int c1, const CtxRunRule &rule, int spec_entry, DevBuf<int32_t> &d_start, DevBuf<int32_t> &d_stop,
                             size_t have, int64_t *row_off, uint32_t *n_out_p) {
    vpr_handle *h = W.h;
    const int64_t n_blk = (nw + 255) / 256;
    const int min_run = rule.min_run, p = rule.p, prim = rule.primitive ? rule.p : 0, min_len = rule.min_len, max_len = rule.max_len;
    uint32_t *d_nkept = as<uint32_t>(W.small);
    uint32_t n_run = 0, n_run_en = 0, n_out = 0;
    *n_out_p = 0;
    if (int rc = W.seg_begin()) return rc;
    if (nw) {
        if (int rc = W.need(W.cnt, size_t(n_blk + 1) * 16, "workgroup counts")) return rc;
        uint32_t *cnt_st = as<uint32_t>(W.cnt), *cnt_en = cnt_st + (n_blk + 1), *off_st = cnt_en + (n_blk + 1), *off_en = off_st + (n_blk + 1);
        HIPCHK(h, hipMemsetAsync(cnt_st + n_blk, 0, 4, h->stream));
        HIPCHK(h, hipMemsetAsync(cnt_en + n_blk, 0, 4, h->stream));
        hipLaunchKernelGGL(k_ctx_run_count, dim3(unsigned(n_blk)), dim3(256), 0, h->stream, words, nw, T0, d_ctg, n_ctg, g0, min_run, cnt_st, cnt_en);
        HIPCHK(h, hipGetLastError());
        if (int rc = scan_u32(W, cnt_st, off_st, size_t(n_blk + 1))) return rc;
        if (int rc = scan_u32(W, cnt_en, off_en, size_t(n_blk + 1))) return rc;
        HIPCHK(h, hipMemcpyAsync(&n_run, off_st + n_blk, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&n_run_en, off_en + n_blk, 4, hipMemcpyDeviceToHost, h->stream));
        if (int rc = W.seg_end()) return rc;
        if (n_run != n_run_en) return fail(h, VPR_ERR_DEVICE, "%s: entry %d: %u run starts and %u run ends", W.entry, spec_entry, n_run, n_run_en);
        if (n_run) {
            const size_t n1 = size_t(n_run) + 1;
            if (int rc = W.need(W.runs, n1 * 8, "run lists")) return rc;
            if (int rc = W.need(W.keep, n1 * 8, "tract flags")) return rc;
            if (int rc = W.need(W.kept, n1 * 12, "kept tracts")) return rc;
            uint32_t *run_st = as<uint32_t>(W.runs), *run_en = run_st + n1;
            uint32_t *flag = as<uint32_t>(W.keep), *flag_scan = flag + n1;
            int32_t *k_ctg = as<int32_t>(W.kept), *k_ps = k_ctg + n1, *k_pe = k_ps + n1;
            if (int rc = W.seg_begin()) return rc;
            hipLaunchKernelGGL(k_ctx_run_write, dim3(unsigned(n_blk)), dim3(256), 0, h->stream, words, nw, T0, d_ctg, n_ctg, g0, min_run, off_st, off_en,
                               run_st, run_en);
            HIPCHK(h, hipGetLastError());
            hipLaunchKernelGGL(k_ctx_keep, dim3(blocks_of(int64_t(n1))), dim3(256), 0, h->stream, int64_t(n_run), run_st, run_en, T0, d_seq, d_ctg,
                               n_ctg, p, prim, min_len, max_len, rule.slop, flag);
            HIPCHK(h, hipGetLastError());
            if (int rc = scan_u32(W, flag, flag_scan, n1)) return rc;
            hipLaunchKernelGGL(k_ctx_compact, dim3(blocks_of(n_run)), dim3(256), 0, h->stream, int64_t(n_run), run_st, run_en, T0, d_seq, d_ctg,
                               n_ctg, p, prim, min_len, max_len, rule.slop, flag, flag_scan, k_ctg, k_ps, k_pe, d_nkept);
            HIPCHK(h, hipGetLastError());
            hipLaunchKernelGGL(k_ctx_group, dim3(blocks_of(int64_t(n1))), dim3(256), 0, h->stream, int64_t(n_run), d_nkept, k_ctg, k_ps, k_pe, flag);
            HIPCHK(h, hipGetLastError());
            if (int rc = scan_u32(W, flag, flag_scan, n1)) return rc;
            HIPCHK(h, hipMemcpyAsync(&n_out, flag_scan + n_run, 4, hipMemcpyDeviceToHost, h->stream));
            if (int rc = W.seg_end()) return rc;
            const size_t want = have + n_out;
            if (int rc = ctx_need(h, W.entry, d_start, want * 4, "intervals", have * 4)) return rc;
            if (int rc = ctx_need(h, W.entry, d_stop, want * 4, "intervals", have * 4)) return rc;
            if (int rc = W.need(W.out_ctg, (size_t(n_out) + 1) * 4, "interval contigs")) return rc;
            if (int rc = W.seg_begin()) return rc;
            if (n_out) {
                hipLaunchKernelGGL(k_ctx_merge, dim3(blocks_of(n_run)), dim3(256), 0, h->stream, d_nkept, k_ctg, k_ps, k_pe, flag, flag_scan,
                                   as<int32_t>(W.out_ctg), d_start.p + have, d_stop.p + have);
                HIPCHK(h, hipGetLastError());
            }
        }
    }
    if (int rc = W.need(W.out_ctg, 4, "interval contigs")) return rc;
    if (int rc = W.seg_begin()) return rc;
    hipLaunchKernelGGL(k_ctx_rows, dim3(blocks_of(c1 - c0 + 1)), dim3(256), 0, h->stream, as<int32_t>(W.out_ctg), int64_t(n_out), c0, c1,
                       int64_t(have), row_off);
    HIPCHK(h, hipGetLastError());
    *n_out_p = n_out;
    return VPR_OK;
}

void context_free(vpr_handle *h) {
    ContextState *S = h->context;
    if (!S) return;
    (void)hipStreamSynchronize(h->stream);
    dev_release(h, S->d_off, S->d_start, S->d_stop);
    for (int k = 0; k < 2; k++) if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
    delete S;
    h->context = nullptr;
}

extern "C" {

int vpr_context_default(const vpr_context_stratum **spec, const char *const **names, int32_t *n) {
    if (!spec || !names || !n) return VPR_ERR_ARG;
    *spec = DEFAULT_SPEC; *names = DEFAULT_NAMES; *n = int32_t(sizeof(DEFAULT_SPEC) / sizeof(DEFAULT_SPEC[0]));
    return VPR_OK;
}

int vpr_context_masks(vpr_handle *h, const vpr_variants *v, const vpr_strata *bed, const vpr_context_stratum *spec, int32_t n_spec) {
    if (!h) return VPR_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    context_free(h);                     // the intervals of the last call end with this one, whatever becomes of it
    if (!v || !spec) return fail(h, VPR_ERR_ARG, "vpr_context_masks: null argument");
    if (n_spec < 1 || n_spec > VPR_CTX_MAX_SPEC) return fail(h, VPR_ERR_ARG, "vpr_context_masks: n_spec %d is not in 1..%d", n_spec, VPR_CTX_MAX_SPEC);
    if (int rc = check_spec(h, spec, n_spec)) return rc;
    const int n_ctg = v->n_ctg;
    if (n_ctg < 1 || !v->ctg_off) return fail(h, VPR_ERR_ARG, "vpr_context_masks: the variants name no contig");
    if (v->ctg_off[0] != 0) return fail(h, VPR_ERR_ARG, "vpr_context_masks: ctg_off[0] is not 0");
    for (int c = 0; c < n_ctg; c++) {
        const int64_t L = v->ctg_off[c + 1] - v->ctg_off[c];
        if (L < 0 || L > INT32_MAX) return fail(h, VPR_ERR_ARG, "vpr_context_masks: contig %d has %lld bases", c, (long long)L);
    }
    const int64_t N = v->ctg_off[n_ctg];
    if (N && !v->ctg_seq) return fail(h, VPR_ERR_ARG, "vpr_context_masks: null ctg_seq");
    if (int rc = strata_check(h, v, bed)) return rc;

    ContextState *S = h->context = new ContextState();
    for (int k = 0; k < 2; k++) HIPCHK(h, hipEventCreate(&S->ev[k]));
    const int n_bed = bed ? bed->n_strata : 0;
    const size_t bed_rows = size_t(n_bed) * size_t(n_ctg), all_rows = bed_rows + size_t(n_spec) * size_t(n_ctg);
    const int64_t n_iv_bed = bed ? bed->iv_off[bed_rows] : 0;
    S->n_spec = n_spec; S->n_ctg = n_ctg; S->n_bed = n_bed; S->n_iv_bed = n_iv_bed;
    const char *const entry = "vpr_context_masks";
    if (int rc = ctx_need(h, entry, S->d_off, 8 * (all_rows + 1), "row offsets")) return rc;
    const size_t iv0 = size_t(n_iv_bed) + 1024;
    if (int rc = ctx_need(h, entry, S->d_start, 4 * iv0, "intervals")) return rc;
    if (int rc = ctx_need(h, entry, S->d_stop, 4 * iv0, "intervals")) return rc;
    if (bed) {
        HIPCHK(h, hipMemcpyAsync(S->d_off.p, bed->iv_off, 8 * (bed_rows + 1), hipMemcpyHostToDevice, h->stream));
        if (n_iv_bed) {
            HIPCHK(h, hipMemcpyAsync(S->d_start.p, bed->iv_start, 4 * size_t(n_iv_bed), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(S->d_stop.p, bed->iv_stop, 4 * size_t(n_iv_bed), hipMemcpyHostToDevice, h->stream));
        }
    }

    CtxWork W(h, entry);
    // the sequence, padded with zero bytes (not called) to whole tiles plus one, so that every 16-byte load stays inside
    const int64_t n_pad = (N + CTX_TILE - 1) / CTX_TILE * CTX_TILE + CTX_TILE;
    if (int rc = W.need(W.seq, size_t(n_pad), "contig sequences")) return rc;
    if (int rc = W.need(W.ctg_off, 8 * (size_t(n_ctg) + 1), "contig offsets")) return rc;
    if (int rc = W.need(W.small, 256, "counters")) return rc;
    if (N) HIPCHK(h, hipMemcpyAsync(W.seq.p, v->ctg_seq, size_t(N), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(as<uint8_t>(W.seq) + N, 0, size_t(n_pad - N), h->stream));
    HIPCHK(h, hipMemcpyAsync(W.ctg_off.p, v->ctg_off, 8 * (size_t(n_ctg) + 1), hipMemcpyHostToDevice, h->stream));
    const uint8_t *d_seq = as<uint8_t>(W.seq);
    const int64_t *d_ctg = as<int64_t>(W.ctg_off);

    const std::vector<CtxPiece> pieces = ctx_pieces(v->ctg_off, n_ctg);

    double ms = 0;
    W.ev[0] = S->ev[0]; W.ev[1] = S->ev[1]; W.ms = &ms;
    HIPCHK(h, x_sync(h, h->stream, SITE));       // (the uploads are not part of the interval kernels' time)

    int64_t n_ctx = 0;
    for (int k = 0; k < n_spec; k++) {
        const vpr_context_stratum &sp = spec[k];
        const bool gc = sp.kind == VPR_CTX_GC;
        // flags a run must have for its tract to reach min_len, where the run passes can apply that themselves (run_masks)
        const int min_run = (!gc && sp.min_len - sp.period <= 64) ? sp.min_len - sp.period : 1;
        int64_t *row_off = S->d_off.p + bed_rows + size_t(k) * size_t(n_ctg);
        for (const CtxPiece &pc : pieces) {
            const int64_t g0 = v->ctg_off[pc.c0], g1 = v->ctg_off[pc.c1], T0 = g0 / CTX_TILE * CTX_TILE;
            const int64_t n_tiles = (g1 - T0 + CTX_TILE - 1) / CTX_TILE, nw = n_tiles * (CTX_TILE / 64);
            uint32_t n_out = 0;
            if (int rc = W.seg_begin()) return rc;
            if (n_tiles) {
                if (int rc = W.need(W.bits, size_t(nw) * 8, "flag bits")) return rc;
                uint16_t *bits = as<uint16_t>(W.bits);
                if (gc) {
                    if (sp.window <= GC_LDS_MAX_W)
                        hipLaunchKernelGGL(k_ctx_flags_gc, dim3(unsigned(n_tiles)), dim3(CTX_WG), size_t(4) * size_t(CTX_TILE + sp.window + 48), h->stream,
                                           d_seq, n_pad, d_ctg, n_ctg, T0, g0, g1, sp.window, sp.gc_lo, sp.gc_hi, as<uint64_t>(W.bits));
                    else
                        hipLaunchKernelGGL(k_ctx_flags_gc_wide, dim3(unsigned(n_tiles)), dim3(CTX_WG), 0, h->stream, d_seq, n_pad, d_ctg, n_ctg, T0, g0, g1,
                                           sp.window, sp.gc_lo, sp.gc_hi, bits);
                } else {
                    switch (sp.period) {
                    case 1: launch_period<1>(unsigned(n_tiles), h->stream, d_seq, d_ctg, n_ctg, T0, g0, g1, bits); break;
                    case 2: launch_period<2>(unsigned(n_tiles), h->stream, d_seq, d_ctg, n_ctg, T0, g0, g1, bits); break;
                    case 3: launch_period<3>(unsigned(n_tiles), h->stream, d_seq, d_ctg, n_ctg, T0, g0, g1, bits); break;
                    case 4: launch_period<4>(unsigned(n_tiles), h->stream, d_seq, d_ctg, n_ctg, T0, g0, g1, bits); break;
                    case 5: launch_period<5>(unsigned(n_tiles), h->stream, d_seq, d_ctg, n_ctg, T0, g0, g1, bits); break;
                    default: launch_period<6>(unsigned(n_tiles), h->stream, d_seq, d_ctg, n_ctg, T0, g0, g1, bits); break;
                    }
                }
                HIPCHK(h, hipGetLastError());
            }
            const CtxRunRule rule = {gc ? 0 : sp.period, gc ? 1 : sp.min_len, gc ? 0 : sp.max_len, sp.slop, min_run, !gc};
            if (int rc = ctx_intervals_from_flags(W, as<uint64_t>(W.bits), nw, T0, g0, d_seq, d_ctg, n_ctg, pc.c0, pc.c1, rule, k, S->d_start, S->d_stop,
                                                  size_t(n_iv_bed + n_ctx), row_off, &n_out))
                return rc;
            n_ctx += n_out;
        }
    }
    if (W.open) if (int rc = W.seg_end()) return rc;
    S->n_iv_ctx = n_ctx;
    S->ms_intervals = ms;
    if (int rc = strata_masks_device(h, v, n_bed + n_spec, S->d_off.p, S->d_start.p, S->d_stop.p)) return rc;
    double ms_hist = 0;
    (void)vpr_strata_timing(h, &S->ms_mask, &ms_hist);
    S->valid = true;
    return VPR_OK;
}

int vpr_context_interval_counts(vpr_handle *h, int64_t *iv_off) {
    if (!h || !iv_off) return VPR_ERR_ARG;
    const ContextState *S = h->context;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_context_interval_counts before vpr_context_masks");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t bed_rows = size_t(S->n_bed) * size_t(S->n_ctg), rows = size_t(S->n_spec) * size_t(S->n_ctg);
    HIPCHK(h, hipMemcpyAsync(iv_off, S->d_off.p + bed_rows, 8 * (rows + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    for (size_t r = 0; r <= rows; r++) iv_off[r] -= S->n_iv_bed;
    return VPR_OK;
}

int vpr_context_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop) {
    if (!h) return VPR_ERR_ARG;
    const ContextState *S = h->context;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_context_download_intervals before vpr_context_masks");
    if (!S->n_iv_ctx) return VPR_OK;
    if (!start || !stop) return fail(h, VPR_ERR_ARG, "vpr_context_download_intervals: null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(start, S->d_start.p + S->n_iv_bed, 4 * size_t(S->n_iv_ctx), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(stop, S->d_stop.p + S->n_iv_bed, 4 * size_t(S->n_iv_ctx), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    return VPR_OK;
}

int vpr_context_info(const vpr_handle *h, int32_t *bases_per_workgroup, int32_t *bases_per_lane) {
    (void)h;                          // (a property of the build: a null handle is accepted)
    if (!bases_per_workgroup || !bases_per_lane) return VPR_ERR_ARG;
    *bases_per_workgroup = CTX_TILE; *bases_per_lane = CTX_LANE;
    return VPR_OK;
}

int vpr_context_timing(const vpr_handle *h, double *ms_intervals, double *ms_mask) {
    if (!h || !ms_intervals || !ms_mask) return VPR_ERR_ARG;
    if (!h->context || !h->context->valid) { *ms_intervals = *ms_mask = 0; return VPR_OK; }
    *ms_intervals = h->context->ms_intervals; *ms_mask = h->context->ms_mask;
    return VPR_OK;
}

}  // extern "C"
