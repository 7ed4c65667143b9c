// pr_nearrepeats.hip -- the near-repeat strata (include/vcfdist_nearrepeats.h): sorted interval lists per (stratum, contig) of the
// bases covered by a k-mer that occurs again in the genome, on either strand, with at most m substitutions.
//
// Equality classes are gone with m > 0, so the sort-and-compare-neighbours of pr_repeats.hip does not apply.  What is left of it is
// the pigeonhole: of the m + 1 fixed blocks of the k bases, two k-mers within m mismatches agree on all bases of at least one.  Per
// stratum (k, m, slop), on the host scaffold KmerWork (pr_kmer.h):
//   1. k_rep_pack<., true> (pr_repeats.hip)   (F, global start) of the valid starts, F the forward code; kept over the blocks
//   per block j of m + 1, one behind the other on the handle's stream:
//   2. k_near_keys                            two records per valid start g: F(g) and RC(g) (computed from F, never stored), each
//                                             rotated by whole bases (Hamming distances keep) so that the block's bases are the
//                                             key's low 2w bits; the value is start << 1 | strand
//   3. vplan_sort_pairs_u64 (pr_plan.hip)     over key bits [0, 2w) only, w <= 16 for m >= 1
//   4. k_near_probe                           a wave takes 64 consecutive sorted records.  The union of their runs of equal block
//                                             key is one contiguous range [lo, hi) of the sorted array (one galloping lower and one
//                                             upper bound per wave).  The wave streams that range 64 partners at a time, one load a
//                                             lane, and every forward record not flagged yet tests every partner of its own run --
//                                             found by a cross-lane read, popcount(((x | x >> 1) & 0x5555...)) of x = a ^ b -- but
//                                             the records of its own start.  ham(F(g), F(h)) is the test against h's forward record,
//                                             ham(F(g), RC(h)) the one against its reverse-complement record, so the forward records
//                                             alone probe.  A record flags only itself, at its k-mer's LAST base as k_rep_mark does;
//                                             the wave stops when all its probing lanes are flagged or the range ends.
//   5. k_rep_piece_words, ctx_intervals_from_flags   the rows, as for the repeat strata (KmerWork::rows_of_entry)
// A record flagged by an earlier block does not probe again but still serves as a partner; since a flag bit is only ever set by
// its own record's lane, the skip reads nothing another lane of the same launch writes: flags, compares and the longest run are
// the same in every run of a call.  There is no cap on a run's length: a record without a partner scans its whole run.
//
// Limits and device memory: the header's.  The buckets KmerState::ms[0..3] are pack, sort (keys and sort), probe, intervals.
#include "pr_kmer.h"
#include "pr_ctxdev.h"
#include "../../include/vcfdist_nearrepeats.h"

struct NearRepeatState : KmerState {
    std::vector<int64_t> n_compares, max_run;          // [n_spec]
};

namespace {

const char *const ENTRY = "vpr_nearrepeat_intervals";
const int NREP_MIN_BLOCK = 8;                          // bases of a block at least: k >= 8 (m + 1)
const int64_t NREP_MAX_BASES = INT32_MAX;              // start << 1 | strand is a 32-bit value
const unsigned PROBE_MAX_WG = 8192;                    // workgroups of the probe kernel (k_near_probe)

// the packed forward pairs of an entry, kept while its blocks' records are built from them
struct NearBufs {
    vpr_handle *h;
    DevBuf<uint8_t> code, start;
    explicit NearBufs(vpr_handle *h_) : h(h_) {}
    ~NearBufs() {
        (void)hipStreamSynchronize(h->stream);
        dev_release(h, code, start);
    }
};

// the code of the reverse complement from the forward code: the pairs of bits reversed, complemented, moved down to bit 0
__device__ inline uint64_t near_rc(uint64_t f, int k) {
    uint64_t x = __brevll(f);
    x = ((x & 0x5555555555555555ull) << 1) | ((x >> 1) & 0x5555555555555555ull);
    return ~x >> (64 - 2 * k);
}

// a code of 2k bits rotated right by r bits, 0 <= r < 2k
__device__ inline uint64_t near_rot(uint64_t x, int k, int r) {
    if (r == 0) return x;
    const uint64_t mask = k == 32 ? ~uint64_t(0) : (uint64_t(1) << (2 * k)) - 1;
    return ((x >> r) | (x << (2 * k - r))) & mask;
}

__device__ inline uint64_t near_lane64(uint64_t v, int lane) {
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), lane));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), lane));
    return (uint64_t(hi) << 32) | lo;
}

}  // namespace

extern "C" {

// records i (forward) and n + i (reverse complement) of valid start i, the block in the low bits of the rotated code
__global__ void __launch_bounds__(256) k_near_keys(const uint64_t *__restrict__ code, const uint32_t *__restrict__ start, uint32_t n, int k, int rot,
                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t f = code[i];
    const uint32_t s = start[i];
    keys[i] = near_rot(f, k, rot); vals[i] = s << 1;
    keys[uint64_t(n) + i] = near_rot(near_rc(f, k), k, rot); vals[uint64_t(n) + i] = (s << 1) | 1u;
}

// The probe over the n2 < 2^32 sorted records (keys: the rotated codes, sorted over the bits of bmask; vals: start << 1 | strand).
// counters: [0] starts newly flagged, [1] compares, [2] the longest run of equal block keys.  256 threads are four independent waves;
// a grid of at most PROBE_MAX_WG workgroups strides over the tiles of 64 records, as k_rep_mark's does over its elements.
__global__ void __launch_bounds__(256) k_near_probe(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n2, int k, int m,
                                                    uint64_t bmask, uint32_t *flags32, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    unsigned long long cmp = 0, longest = 0, flagged = 0;                        // the wave's sums over its tiles (flagged: the same in every lane)
    for (uint64_t b64 = (uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * 64; b64 < n2; b64 += uint64_t(gridDim.x) * 256) {      // (the whole wave)
        const uint32_t b = uint32_t(b64);
        const int cnt = n2 - b < 64u ? int(n2 - b) : 64;
        const bool have = lane < cnt;
        const uint64_t key = have ? keys[b + lane] : 0;
        const uint32_t val = have ? vals[b + lane] : 0;
        const uint64_t bk = key & bmask;
        const uint64_t bk_first = near_lane64(bk, 0), bk_last = near_lane64(bk, __builtin_amdgcn_readfirstlane(cnt - 1));

        // [lo, hi): from the first record with the wave's first block key to behind the last with its last; galloping, since most runs
        // are short and end beside the wave
        uint32_t lo, hi;
        {
            uint32_t top = b, s = 1;                                                 // the record at top has bk_first
            while (top >= s && (keys[top - s] & bmask) == bk_first) { top -= s; s *= 2; }
            uint32_t l = top >= s ? top - s + 1 : 0, r = top;                        // the first such record is in [l, r]
            while (l < r) { const uint32_t mid = l + (r - l) / 2; if ((keys[mid] & bmask) < bk_first) l = mid + 1; else r = mid; }
            lo = l;
            uint32_t bot = b + uint32_t(cnt) - 1;                                    // the record at bot has bk_last
            s = 1;
            while (n2 - 1 - bot >= s && (keys[bot + s] & bmask) == bk_last) { bot += s; s *= 2; }
            l = bot + 1; r = n2 - 1 - bot >= s ? bot + s : n2;                       // the first record behind the run is in [l, r]
            while (l < r) { const uint32_t mid = l + (r - l) / 2; if ((keys[mid] & bmask) <= bk_last) l = mid + 1; else r = mid; }
            hi = l;
        }

        // the lane's own run [run_lo, run_hi) from the run heads inside the wave and the two bounds
        const uint32_t up_lo = uint32_t(__shfl_up(int(uint32_t(bk)), 1)), up_hi = uint32_t(__shfl_up(int(uint32_t(bk >> 32)), 1));
        const bool head = have && (lane == 0 || ((uint64_t(up_hi) << 32) | up_lo) != bk);
        const uint64_t heads = __ballot(head);
        const uint64_t upto = lane == 63 ? ~uint64_t(0) : (uint64_t(2) << lane) - 1;     // bits 0..lane
        const int first = 63 - __clzll((long long)(heads & upto));                        // (bit 0 is set)
        const uint64_t behind = heads & ~upto;
        const int next = behind ? __ffsll((long long)behind) - 1 : cnt;
        const uint32_t run_lo = first == 0 ? lo : b + uint32_t(first);
        const uint32_t run_hi = next == cnt ? hi : b + uint32_t(next);

        const uint32_t mystart = val >> 1;
        const uint64_t pos = uint64_t(mystart) + uint64_t(k - 1);
        const bool active = have && !(val & 1u) && !((flags32[pos >> 5] >> (pos & 31)) & 1u);
        bool found = false;
        uint32_t compares = 0;                                                       // (a lane tests at most its run, below 2^32 records)
        if (__ballot(active)) {
            for (uint64_t base = lo; base < hi; base += 64) {
                const bool want = active && !found;
                if (!__ballot(want)) break;
                if (!__ballot(want && uint64_t(run_lo) < base + 64 && uint64_t(run_hi) > base)) continue;     // (no probing lane's run is here)
                const uint64_t p = base + uint64_t(lane);
                const uint64_t pk = p < hi ? keys[p] : 0;
                const uint32_t pv = p < hi ? vals[p] : 0;
#pragma unroll
                for (int q = 0; q < 64; q++) {
                    const uint64_t qk = near_lane64(pk, q);
                    const uint32_t qs = uint32_t(__builtin_amdgcn_readlane(int(pv), q)) >> 1;
                    const uint64_t at = base + uint64_t(q);                              // (behind hi: in no lane's run)
                    if (want && !found && at >= run_lo && at < run_hi && qs != mystart) {
                        const uint64_t x = key ^ qk;
                        compares++;
                        if (__popcll((x | (x >> 1)) & 0x5555555555555555ull) <= m) found = true;
                    }
                }
            }
        }
        if (found) atomicOr(&flags32[pos >> 5], 1u << (pos & 31));

        cmp += compares;
        if (have && run_hi - run_lo > longest) longest = run_hi - run_lo;
        flagged += (unsigned long long)__popcll(__ballot(found));
    }
    // one add per counter and wave: the adds go to ONE address each, and one per tile of 64 records took longer than the probe itself
    for (int d = 32; d; d >>= 1) {
        cmp += __shfl_xor(cmp, d);
        const unsigned long long o = __shfl_xor(longest, d);
        longest = o > longest ? o : longest;
    }
    if (lane == 0) {
        if (flagged) atomicAdd(&counters[0], flagged);
        if (cmp) atomicAdd(&counters[1], cmp);
        if (longest) atomicMax(&counters[2], longest);
    }
}

}  // extern "C"

void nearrepeats_free(vpr_handle *h) { kmer_free(h, &vpr_handle::nearrepeats); }

extern "C" {

int vpr_nearrepeat_name(const vpr_near_stratum *spec, char *buf, size_t size) {
    if (!spec || !buf) return VPR_ERR_ARG;
    const int n = snprintf(buf, size, "near_k%d_m%d", int(spec->k), int(spec->m));
    return n < 0 || size_t(n) >= size ? VPR_ERR_ARG : VPR_OK;
}

int vpr_nearrepeat_intervals(vpr_handle *h, int32_t n_ctg, const int64_t *ctg_off, const uint8_t *ctg_seq, const vpr_near_stratum *spec,
                             int32_t n_spec) {
    if (!h) return VPR_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    nearrepeats_free(h);                 // the intervals of the last call end with this one, whatever becomes of it
    if (!spec) return fail(h, VPR_ERR_ARG, "%s: null spec", ENTRY);
    if (n_spec < 1 || n_spec > VPR_NREP_MAX_SPEC) return fail(h, VPR_ERR_ARG, "%s: n_spec %d is not in 1..%d", ENTRY, n_spec, VPR_NREP_MAX_SPEC);
    std::vector<vpr_repeat_stratum> ks(size_t(n_spec), vpr_repeat_stratum{0, 0});          // what the scaffold's checks read
    for (int e = 0; e < n_spec; e++) {
        if (spec[e].m < 0 || spec[e].m > VPR_NREP_MAX_M)
            return fail(h, VPR_ERR_ARG, "%s: entry %d: m %d is not in 0..%d", ENTRY, e, spec[e].m, VPR_NREP_MAX_M);
        if (spec[e].k < NREP_MIN_BLOCK * (spec[e].m + 1) || spec[e].k > VPR_NREP_MAX_K)
            return fail(h, VPR_ERR_ARG, "%s: entry %d: k %d is not in %d..%d at m %d", ENTRY, e, spec[e].k, NREP_MIN_BLOCK * (spec[e].m + 1),
                        VPR_NREP_MAX_K, spec[e].m);
        for (int f = 0; f < e; f++)
            if (spec[f].k == spec[e].k && spec[f].m == spec[e].m && spec[f].slop == spec[e].slop)
                return fail(h, VPR_ERR_ARG, "%s: entries %d and %d are equal", ENTRY, f, e);
        ks[size_t(e)] = vpr_repeat_stratum{spec[e].k, spec[e].slop};
    }
    if (int rc = KmerWork::check_args(h, ENTRY, NREP_MIN_BLOCK, VPR_NREP_MAX_K, VPR_NREP_MAX_SPEC, n_ctg, ctg_off, ctg_seq, ks.data(), n_spec)) return rc;
    if (ctg_off[n_ctg] > NREP_MAX_BASES)
        return fail(h, VPR_ERR_ARG, "%s: %lld bases in total, above the %lld that a 31-bit start beside the strand bit can name", ENTRY,
                    (long long)ctg_off[n_ctg], (long long)NREP_MAX_BASES);
    NearRepeatState *S = h->nearrepeats = new NearRepeatState();
    if (int rc = S->init(h, n_spec, n_ctg)) return rc;
    S->n_compares.assign(size_t(n_spec), 0); S->max_run.assign(size_t(n_spec), 0);
    KmerWork K(h, ENTRY);
    NearBufs B(h);
    CtxWork &W = K.W;
    if (int rc = K.upload(n_ctg, ctg_off, ctg_seq, size_t(n_spec) * size_t(n_ctg))) return rc;
    if (int rc = K.begin_timing(S)) return rc;

    int64_t n_iv = 0;
    for (int e = 0; e < n_spec; e++) {
        const int k = spec[e].k, m = spec[e].m;
        uint32_t n = 0;                  // valid starts (at most N < 2^31, so that 2 n records have 32-bit indices)
        unsigned long long counters[3] = {0, 0, 0};
        if (K.n_tiles) {
            W.ms = &S->ms[0];
            if (int rc = W.seg_begin()) return rc;
            if (int rc = K.pack(k, &n, true)) return rc;
            if (int rc = W.seg_end()) return rc;
        }
        S->n_valid[size_t(e)] = int64_t(n);
        HIPCHK(h, hipMemsetAsync(K.flags.p, 0, size_t(K.nw) * 8 + 8, h->stream));
        if (n) {
            // the packed pairs move aside, and the room for both strands' records and their sort is made, under no clock
            const size_t n2 = 2 * size_t(n);
            if (int rc = K.need(B.code, size_t(n) * 8, "forward codes")) return rc;
            if (int rc = K.need(B.start, size_t(n) * 4, "forward starts")) return rc;
            HIPCHK(h, hipMemcpyAsync(B.code.p, K.keys.p, size_t(n) * 8, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(B.start.p, K.vals.p, size_t(n) * 4, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemsetAsync(K.d_count, 0, sizeof counters, h->stream));
            HIPCHK(h, x_sync(h, h->stream, SITE));
            if (int rc = K.pair_room(n2)) return rc;
            for (int j = 0; j <= m; j++) {
                const int b0 = j * k / (m + 1), b1 = (j + 1) * k / (m + 1), w = b1 - b0;
                W.ms = &S->ms[1];
                if (int rc = K.sort_room(n2, unsigned(2 * w))) return rc;
                if (int rc = W.seg_begin()) return rc;
                hipLaunchKernelGGL(k_near_keys, dim3(blocks_of(int64_t(n))), dim3(256), 0, h->stream, as<uint64_t>(B.code), as<uint32_t>(B.start), n, k,
                                   2 * (k - b1), as<uint64_t>(K.keys), as<uint32_t>(K.vals));
                HIPCHK(h, hipGetLastError());
                if (int rc = K.sort(n2, unsigned(2 * w))) return rc;
                if (int rc = W.seg_end()) return rc;
                W.ms = &S->ms[2];
                if (int rc = W.seg_begin()) return rc;
                const uint64_t bmask = w == 32 ? ~uint64_t(0) : (uint64_t(1) << (2 * w)) - 1;
                hipLaunchKernelGGL(k_near_probe, dim3(std::min(blocks_of(int64_t(n2)), PROBE_MAX_WG)), dim3(256), 0, h->stream, K.keys_out, K.vals_out, uint32_t(n2), k, m, bmask,
                                   as<uint32_t>(K.flags), K.d_count);
                HIPCHK(h, hipGetLastError());
                if (j == m) HIPCHK(h, hipMemcpyAsync(counters, K.d_count, sizeof counters, hipMemcpyDeviceToHost, h->stream));
                if (int rc = W.seg_end()) return rc;
            }
        }
        S->n_repeated[size_t(e)] = int64_t(counters[0]); S->n_compares[size_t(e)] = int64_t(counters[1]); S->max_run[size_t(e)] = int64_t(counters[2]);
        W.ms = &S->ms[3];
        if (int rc = K.rows_of_entry(k, spec[e].slop, e, e, &n_iv)) return rc;
    }
    if (int rc = K.download_rows(n_iv, S->off, S->start, S->stop)) return rc;
    S->valid = true;
    return VPR_OK;
}

int vpr_nearrepeat_interval_counts(vpr_handle *h, int64_t *iv_off) {
    return h ? kmer_interval_counts(h, h->nearrepeats, "vpr_nearrepeat_interval_counts", ENTRY, iv_off) : VPR_ERR_ARG;
}

int vpr_nearrepeat_download_intervals(vpr_handle *h, int32_t *start, int32_t *stop) {
    return h ? kmer_download_intervals(h, h->nearrepeats, "vpr_nearrepeat_download_intervals", ENTRY, start, stop) : VPR_ERR_ARG;
}

int vpr_nearrepeat_stats(vpr_handle *h, int64_t *n_valid, int64_t *n_near, int64_t *n_compares, int64_t *max_run) {
    if (!h) return VPR_ERR_ARG;
    const NearRepeatState *S = h->nearrepeats;
    if (int rc = kmer_stats(h, S, "vpr_nearrepeat_stats", ENTRY, n_compares && max_run, n_valid, n_near)) return rc;
    std::copy(S->n_compares.begin(), S->n_compares.end(), n_compares);
    std::copy(S->max_run.begin(), S->max_run.end(), max_run);
    return VPR_OK;
}

int vpr_nearrepeat_timing(const vpr_handle *h, double *ms_pack, double *ms_sort, double *ms_probe, double *ms_intervals) {
    return h ? kmer_timing(h->nearrepeats, ms_pack, ms_sort, ms_probe, ms_intervals) : VPR_ERR_ARG;
}

}  // extern "C"
