// pr_swg.h -- the affine-gap wavefront alignment with a band-compacted history and its backtrack, shared by the distance metrics
// (pr_dist.hip) and the realignment (pr_realign.hip): wf_swg_align (dist.cpp:1510-1652) and wf_swg_backtrack (dist.cpp:2625-2757).
//
// A job's slice of the round arena holds, in order: the reversed query (pad16(q) bytes), the reversed truth / reference
// (pad16(t)), the row headers (16 B each) and the cells (int32 offsets, then uint8 pointer flags in the history pass).  The caller
// decides how a job's two strings are loaded (swg_wave's `load`) and what the walk emits (swg_walk's `emit`).  The host half at
// the end (Rounds) runs the jobs of either step in rounds that fit the arena.
//
// The band: a row's cells can be set only from rows s-x, s-(o+e), s-e one diagonal apart at most, so every row s has a diagonal
// range [lo_s, hi_s] that the previous ranges bound (arithmetic, the same in both passes); a cell outside it is provably never
// written (-2 / no pointer) and is not stored.  The reference loops over all q + t - 1 diagonals.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

namespace swg {

enum { DM_SUB = 0, DM_INS = 1, DM_DEL = 2 };
enum : uint8_t { DP_INS = 1, DP_DEL = 2, DP_MAT = 4, DP_SUB = 8 };          // src/defs.h:110-114

struct DRow { int32_t lo, hi; int64_t base; };                 // diagonal range of a wavefront row, first cell of its slice
struct DPen { int x, o, e; };

__host__ __device__ inline int64_t pad16(int64_t b) { return (b + 15) & ~int64_t(15); }

// pass-1 scratch of a job: both strings, a ring of P row headers and P rows of three full-width matrices
__host__ __device__ inline int64_t need1(int q, int t, int P) {
    return pad16(pad16(q) + pad16(t) + 16 * int64_t(P) + 12 * int64_t(P) * (q + t - 1 > 1 ? q + t - 1 : 1));
}
// pass-2 slice of a job: both strings, s + 1 row headers, the cells and their pointer flags
__host__ __device__ inline int64_t need2(int q, int t, int s, int64_t cells) {
    return pad16(pad16(q) + pad16(t) + 16 * (int64_t(s) + 1) + 4 * cells + pad16(cells));
}

// wavefront rows of one job: a ring of P rows (pass 1) or every row, band-compacted (pass 2)
template <bool HIST>
struct Rows {
    DRow *row;            // [P] or [s + 1]
    int32_t *off;         // cells
    uint8_t *ptr;         // pointer flags (HIST only)
    int P;
    __device__ DRow get(int s) const { return row[HIST ? s : s % P]; }
    // offs[m][r][d] as the reference would read it: -2 outside the row's band or before score 0
    __device__ int ld(int r, int m, int d) const {
        if (r < 0) return -2;
        const DRow R = get(r);
        if (d < R.lo || d > R.hi) return -2;
        return off[R.base + int64_t(m) * (R.hi - R.lo + 1) + (d - R.lo)];
    }
};

struct WaveOut { int s; int64_t cells; bool failed; };

// pass 1 (HIST = false) / pass 2 (HIST = true) of one job, one wavefront of 64 lanes over the diagonals.  base: the job's slice;
// load(qs, ts, lane) fills the reversed strings (q and t bytes); s_hist / cell_cap_hist: what pass 1 returned (HIST only).
// Every lane returns the same WaveOut: the final score, the band-compacted cells a history of it holds, and whether the
// alignment failed (a score beyond any alignment's, or a history beyond what pass 1 sized).
template <bool HIST, typename Load>
__device__ WaveOut swg_wave(int q, int t, DPen pen, uint8_t *base, int s_hist, int64_t cell_cap_hist, Load load) {
    const int lane = threadIdx.x;
    const int mat_len = q + t - 1;
    const int x = pen.x, o = pen.o, e = pen.e, oe = o + e;
    const int P = max(x, oe) + 1;
    uint8_t *qs = base, *ts = base + pad16(q);
    Rows<HIST> R;
    R.P = P;
    R.row = reinterpret_cast<DRow *>(ts + pad16(t));
    const int64_t n_rows = HIST ? int64_t(s_hist) + 1 : P;
    R.off = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(R.row) + 16 * n_rows);
    const int64_t cell_cap = HIST ? cell_cap_hist : int64_t(3) * P * mat_len;
    R.ptr = reinterpret_cast<uint8_t *>(R.off + cell_cap);
    load(qs, ts, lane);
    // a bound no alignment reaches: every base substituted plus every base gapped
    const int64_t s_max = int64_t(x) * (q + t) + int64_t(oe) * (q + t) + 1;

    int s = 0;
    int64_t cells = 3;
    if (lane == 0) {
        R.row[0] = DRow{q - 1, q - 1, 0};
        R.off[DM_SUB] = -1; R.off[DM_INS] = -2; R.off[DM_DEL] = -2;
        if (HIST) { R.ptr[DM_SUB] = DP_MAT; R.ptr[DM_INS] = 0; R.ptr[DM_DEL] = 0; }
    }
    __syncthreads();
    bool failed = false;
    for (;;) {
        const DRow C = R.get(s);
        const int w = C.hi - C.lo + 1;
        // close INS / DEL into SUB (INS first, then DEL), dist.cpp:1532-1546
        for (int d = C.lo + lane; d <= C.hi; d += 64) {
            const int64_t c = C.base + (d - C.lo);
            const int diag = d + 1 - q;
            for (int m = DM_INS; m <= DM_DEL; m++) {
                const int off = R.off[c + int64_t(m) * w];
                if (off >= 0 && off < q && diag + off >= 0 && diag + off < t && off >= R.off[c]) {
                    R.off[c] = off;
                    if (HIST) R.ptr[c] |= (m == DM_INS) ? DP_INS : DP_DEL;
                }
            }
        }
        // extend along the diagonals (SUB only); the reference stops at the first diagonal that finishes
        bool done = false;
        for (int d0 = C.lo; d0 <= C.hi && !done; d0 += 64) {
            const int d = d0 + lane;
            bool fin = false;
            if (d <= C.hi) {
                const int64_t c = C.base + (d - C.lo);
                const int diag = d + 1 - q;
                int off = R.off[c];
                while (off != -2 && diag + off >= -1 && off < q - 1 && diag + off < t - 1 && qs[off + 1] == ts[diag + off + 1]) off++;
                R.off[c] = off;
                fin = off == q - 1 && off + diag == t - 1;
            }
            done = __any(fin);
        }
        if (done) break;
        s++;
        if (s > s_max) { failed = true; break; }
        // the new row's band from the rows it reads
        int lo = INT_MAX, hi = INT_MIN;
        auto widen = [&](int r, int dl, int dh) {
            if (r < 0) return;
            const DRow S = R.get(r);
            if (S.lo > S.hi) return;
            lo = min(lo, S.lo + dl); hi = max(hi, S.hi + dh);
        };
        widen(s - x, 0, 0);
        widen(s - oe, -1, 1);
        widen(s - e, -1, 1);
        lo = max(lo, 0); hi = min(hi, mat_len - 1);
        if (lo > hi) { lo = 1; hi = 0; }
        const int wn = hi - lo + 1;
        const int64_t nb = HIST ? cells : int64_t(s % P) * 3 * mat_len;
        if (HIST && (s > s_hist || cells + 3 * int64_t(wn) > cell_cap)) { failed = true; break; }
        __syncthreads();                  // every lane is done reading the ring slot about to be replaced
        if (lane == 0) R.row[HIST ? s : s % P] = DRow{lo, hi, nb};
        __syncthreads();
        cells += 3 * int64_t(wn);
        for (int d = lo + lane; d <= hi; d += 64) {
            const int diag = d + 1 - q;
            int vs = -2, vd = -2, vi = -2;
            uint8_t fs = 0, fd = 0, fi = 0;
            int p;
            if (s - x >= 0 && (p = R.ld(s - x, DM_SUB, d)) != -2 && p + 1 < q && diag + p + 1 < t && p + 1 >= vs) { vs = p + 1; fs |= DP_SUB; }
            if (s - oe >= 0 && d > 0 && (p = R.ld(s - oe, DM_SUB, d - 1)) != -2 && diag + p < t && p >= vd) { vd = p; fd |= DP_SUB; }
            if (s - oe >= 0 && d < mat_len - 1 && (p = R.ld(s - oe, DM_SUB, d + 1)) != -2 && p + 1 < q && diag + p + 1 < t &&
                diag + p + 1 >= 0 && p + 1 >= vi) { vi = p + 1; fi |= DP_SUB; }
            if (s - e >= 0 && d > 0 && (p = R.ld(s - e, DM_DEL, d - 1)) != -2 && diag + p < t && p >= vd) { vd = p; fd |= DP_DEL; }
            if (s - e >= 0 && d < mat_len - 1 && (p = R.ld(s - e, DM_INS, d + 1)) != -2 && p + 1 < q && diag + p + 1 < t &&
                diag + p + 1 >= 0 && p + 1 >= vi) { vi = p + 1; fi |= DP_INS; }
            const int64_t c = nb + (d - lo);
            R.off[c] = vs; R.off[c + wn] = vi; R.off[c + 2 * int64_t(wn)] = vd;
            if (HIST) { R.ptr[c] = fs; R.ptr[c + wn] = fi; R.ptr[c + 2 * int64_t(wn)] = fd; }
        }
        __syncthreads();
    }
    return WaveOut{s, cells, failed};
}

// wf_swg_backtrack over a job's pass-2 history, one thread.  The strings are reversed, so the walk goes over the forward
// alignment from its start: emit(type, qi, ri) once per step (DP_MAT / DP_SUB: one base of each string, DP_INS: one query base,
// DP_DEL: one truth base) with the step's indices into the REVERSED strings (forward index = length - 1 - index).
// -> false when the walk meets a pointer the reference would ERROR on.
template <typename Emit>
__device__ bool swg_walk(const uint8_t *base, int q, int t, int s_fin, int64_t cells, DPen pen, Emit emit) {
    Rows<true> R;
    R.P = 0;
    R.row = reinterpret_cast<DRow *>(const_cast<uint8_t *>(base) + pad16(q) + pad16(t));
    R.off = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(R.row) + 16 * (int64_t(s_fin) + 1));
    R.ptr = reinterpret_cast<uint8_t *>(R.off + cells);
    auto flag = [&](int r, int m, int d) -> uint8_t {
        if (r < 0) return 0;
        const DRow W = R.get(r);
        if (d < W.lo || d > W.hi) return 0;
        return R.ptr[W.base + int64_t(m) * (W.hi - W.lo + 1) + (d - W.lo)];
    };
    const int x = pen.x, o = pen.o, e = pen.e;
    int qi = q - 1, ri = t - 1, mi = DM_SUB, s = s_fin;
    bool bad = false;
    while ((qi >= 0 || ri >= 0) && !bad) {
        if (s < 0) { bad = true; break; }
        const int d = q - 1 + ri - qi;
        if (mi == DM_SUB) {
            const uint8_t f = flag(s, DM_SUB, d);
            if (f & (DP_INS | DP_DEL)) {              // a gap ends here: INS preferred
                const int m = (f & DP_INS) ? DM_INS : DM_DEL;
                const int prev = R.ld(s, m, d);
                while (qi > prev && !bad) { emit(DP_MAT, qi, ri); qi--; ri--; bad = qi < 0 || ri < 0; }
                mi = m;
            } else if (f & DP_SUB) {
                if (s - x < 0) { bad = true; break; }
                const int prev = R.ld(s - x, DM_SUB, d);
                while (qi > prev + 1 && !bad) { emit(DP_MAT, qi, ri); qi--; ri--; bad = qi < 0 || ri < 0; }
                if (bad) break;
                emit(DP_SUB, qi, ri); qi--; ri--;
                s -= x;
            } else if (f & DP_MAT) {
                while (qi >= 0 && ri >= 0) { emit(DP_MAT, qi, ri); qi--; ri--; }
                if (qi >= 0 || ri >= 0) bad = true;
            } else {
                bad = true;
            }
        } else {
            const uint8_t f = flag(s, mi, d);
            const uint8_t ext = mi == DM_INS ? DP_INS : DP_DEL;
            if (!(f & (ext | DP_SUB))) { bad = true; break; }
            emit(ext, qi, ri);
            if (mi == DM_INS) qi--; else ri--;
            if (f & ext) s -= e;
            else { mi = DM_SUB; s -= o + e; }
        }
        if (!(qi == -1 && ri == -1) && (qi < 0 || ri < 0)) bad = true;
    }
    return !bad;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: the rounds both steps run their jobs in
// ---------------------------------------------------------------------------------------------------------------------
// Pass-1 scratch and pass-2 histories share one round arena.  Pass-1 rounds pack jobs up to cap1 bytes of scratch; inside each,
// pass-2 sub-rounds pack its jobs up to cap2 bytes of history, and every sub-round is followed by the caller's backtrack step while
// its histories are in the arena.  A job larger than its cap runs alone, a job larger than `limit` gets `limit_bit` and never runs,
// a job that already carries a status is skipped.
enum { ROUNDS_OK = 0, ROUNDS_NOMEM, ROUNDS_DEVICE };
#define SWG_TRY(call) do { if ((err = (call)) != hipSuccess) { what = #call; return ROUNDS_DEVICE; } } while (0)
struct Rounds {
    hipStream_t st;
    hipEvent_t ev[2];
    int64_t limit, cap1, cap2;
    uint8_t limit_bit;
    int64_t *d_slice;               // the job columns on the device: arena offset (written here), status (both ways), pass-2 bytes (read here)
    uint8_t *d_status;
    const int64_t *d_need2;
    // what a run leaves: rounds of either level, the peak bytes a round occupied, device time of the three phases, and the call
    // that failed where run() returns ROUNDS_DEVICE of its own
    int64_t n_rounds = 0, n_hist_rounds = 0, arena_bytes = 0;
    double ms_score = 0, ms_hist = 0, ms_back = 0;
    hipError_t err = hipSuccess;
    const char *what = "";

    // need1: the jobs' pass-1 bytes; status: the host copy, kept current.  The caller's pieces, all on `st`:
    //   sync()                       waits for the stream (hipError_t)
    //   arena(bytes)                 an arena of at least `bytes` from the caller's allocator, the previous one released; null: no memory
    //   pass(hist, a, n, arena)      launches pass 1 / pass 2 of jobs [a, a + n)
    //   back(c, m, arena)            the backtrack of sub-round [c, c + m) on the device (timed as ms_back); ROUNDS_*
    //   collect(c, m)                what the host takes from that sub-round before the arena is reused; ROUNDS_*
    template <typename Sync, typename Arena, typename Pass, typename Back, typename Collect>
    int run(const std::vector<int64_t> &need1, std::vector<uint8_t> &status, Sync sync, Arena arena, Pass pass, Back back, Collect collect) {
        const int64_t n_jobs = int64_t(need1.size());
        uint8_t *d_arena = nullptr;
        int64_t arena_cap = 0;
        // greedy round over [a, b): the jobs' slices into `slice` (indexed from off0), -> (end of the round, its bytes)
        auto next_round = [&](const std::vector<int64_t> &need, int64_t a, int64_t b, int64_t off0, std::vector<int64_t> &slice, int64_t cap) {
            int64_t sum = 0, k = a;
            for (; k < b; k++) {
                const int64_t nb = need[size_t(k - off0)];
                slice[size_t(k - off0)] = sum;
                if (status[size_t(k)]) continue;
                if (nb > limit) { status[size_t(k)] = limit_bit; continue; }
                if (sum > 0 && sum + nb > cap) break;
                sum += nb;
            }
            return std::make_pair(k, std::max<int64_t>(sum, 16));
        };
        auto ensure_arena = [&](int64_t bytes) {
            arena_bytes = std::max(arena_bytes, bytes);
            if (bytes > arena_cap) { d_arena = arena(bytes); arena_cap = d_arena ? bytes : 0; }
            return d_arena != nullptr;
        };
        // slices and statuses of jobs [a, a + n) up, the pass, its device time
        auto run_pass = [&](bool hist, int64_t a, int64_t n, const int64_t *slice, double *ms) -> int {
            SWG_TRY(hipMemcpyAsync(d_slice + a, slice, 8 * size_t(n), hipMemcpyHostToDevice, st));
            SWG_TRY(hipMemcpyAsync(d_status + a, status.data() + a, size_t(n), hipMemcpyHostToDevice, st));
            SWG_TRY(hipEventRecord(ev[0], st));
            pass(hist, a, n, d_arena);
            SWG_TRY(hipEventRecord(ev[1], st));
            return hist ? elapsed(ms) : ROUNDS_OK;       // (pass 1 is read after the downloads its round waits for anyway)
        };
        auto status_down = [&](int64_t a, int64_t n) -> int {
            SWG_TRY(hipMemcpyAsync(status.data() + a, d_status + a, size_t(n), hipMemcpyDeviceToHost, st));
            SWG_TRY(sync());
            return ROUNDS_OK;
        };
        std::vector<int64_t> sl1(need1.size()), sl2, n2;
        for (int64_t a = 0; a < n_jobs;) {
            const auto r1 = next_round(need1, a, n_jobs, 0, sl1, cap1);
            const int64_t b = r1.first, nr = b - a;
            n_rounds++;
            if (!ensure_arena(r1.second)) return ROUNDS_NOMEM;
            if (int rc = run_pass(false, a, nr, sl1.data() + a, nullptr)) return rc;
            SWG_TRY(hipGetLastError());
            n2.assign(size_t(nr), 0);
            SWG_TRY(hipMemcpyAsync(n2.data(), d_need2 + a, 8 * size_t(nr), hipMemcpyDeviceToHost, st));
            if (int rc = status_down(a, nr)) return rc;
            if (int rc = elapsed(&ms_score)) return rc;
            sl2.assign(size_t(nr), 0);
            for (int64_t c = a; c < b;) {
                const auto r2 = next_round(n2, c, b, a, sl2, cap2);
                const int64_t m = r2.first - c;
                n_hist_rounds++;
                if (!ensure_arena(r2.second)) return ROUNDS_NOMEM;
                if (int rc = run_pass(true, c, m, sl2.data() + (c - a), &ms_hist)) return rc;
                SWG_TRY(hipEventRecord(ev[0], st));
                if (int rc = back(c, m, d_arena)) return rc;
                SWG_TRY(hipEventRecord(ev[1], st));
                SWG_TRY(hipGetLastError());
                if (int rc = elapsed(&ms_back)) return rc;
                if (int rc = collect(c, m)) return rc;
                c = r2.first;
            }
            if (int rc = status_down(a, nr)) return rc;
            a = b;
        }
        return ROUNDS_OK;
    }
    // *ms += the device time between the two events
    int elapsed(double *ms) {
        float t = 0;
        SWG_TRY(hipEventSynchronize(ev[1]));
        SWG_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        *ms += t;
        return ROUNDS_OK;
    }
};
#undef SWG_TRY

}  // namespace swg
