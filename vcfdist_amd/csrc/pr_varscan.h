// pr_varscan.h -- what the kernels that join hap-variants by position share (k_varstrata_mask, pr_varstrata.hip; k_errclass,
// pr_errclass.hip; k_matchkind, pr_matchkind.hip): the columns of one hap slot, the two bisections over a range of sorted positions, and the test and the scan
// for copies of a variant in the run of equal position.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

// the columns of one hap slot the kernels read (a kernel that never looks at REF bytes leaves ref_off null)
struct VsCols {
    const int64_t *var_off, *ref_off, *alt_off;
    const int32_t *pos, *ref_len, *alt_len;
    const uint8_t *type, *pool;
};

// first index of [lo, hi) whose position is >= key (lower) / > key (upper); the keys are 64-bit so that pos +- W cannot wrap
__device__ __forceinline__ int64_t vs_lower(const int32_t *__restrict__ pos, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (int64_t(pos[mid]) < key) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ int64_t vs_upper(const int32_t *__restrict__ pos, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (int64_t(pos[mid]) <= key) lo = mid + 1; else hi = mid; }
    return lo;
}

// variant u of slot x, known to start where the variant (type, both lengths, ALT bytes at `alt`) starts, is a copy of it; the ALT
// bytes are compared only where everything else agrees
__device__ __forceinline__ bool vs_is_copy(const VsCols &x, int64_t u, uint8_t type, int32_t ref_len, int32_t alt_len,
                                           const uint8_t *__restrict__ alt) {
    if (x.type[u] != type || x.ref_len[u] != ref_len || x.alt_len[u] != alt_len) return false;
    const uint8_t *__restrict__ b = x.pool + x.alt_off[u];
    int32_t j = 0;
    while (j < alt_len && b[j] == alt[j]) j++;
    return j == alt_len;
}

// copies of a variant (pos, type, both lengths, ALT bytes at `alt`) among the variants [lo, hi) of slot x other than index
// `skip`: a scan of the run of equal pos
__device__ __forceinline__ int vs_copies(const VsCols &x, int64_t lo, int64_t hi, int64_t skip, int32_t pos, uint8_t type, int32_t ref_len,
                                         int32_t alt_len, const uint8_t *__restrict__ alt) {
    int n = 0;
    for (int64_t u = vs_lower(x.pos, lo, hi, pos); u < hi && x.pos[u] == pos; u++)
        n += u != skip && vs_is_copy(x, u, type, ref_len, alt_len, alt);
    return n;
}
