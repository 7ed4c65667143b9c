// pr_counts.h -- what the three counter kernels (k_pr_hist, pr_collect.hip; k_pr_hist_strata and k_pr_boot, pr_cut.hip, with their label siblings)
// and the two join kernels (k_errclass, pr_errclass.hip; k_matchkind, pr_matchkind.hip) decide alike: the supercluster of a variant and the bin the variant counts in (print.cpp:328-438).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/vcfdist_pr.h"

// supercluster of variant v: the largest sc with var_off[sc] <= v
__device__ __forceinline__ int sc_of_var(const int64_t *__restrict__ var_off, int n_sc, int64_t v) {
    int lo = 0, hi = n_sc;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (var_off[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}

// The phasing supercluster sc selects, as pr_count_row settles it: 0 the original, 1 the swapped one (for a kernel that needs the
// choice itself, k_errclass and k_matchkind; the counter kernels get it inside pr_count_row)
__device__ __forceinline__ int pr_phase_swap(int sc, const int32_t *__restrict__ sc_phase, const int32_t *__restrict__ pb_phase) {
    const int ph = sc_phase[sc];
    return ph == VPR_PHASE_ORIG ? 0 : (ph == VPR_PHASE_SWAP ? 1 : (pb_phase ? (pb_phase[sc] != 0) : 0));
}

// The (class, errtype) row, class * 3 + errtype, of variant v of supercluster sc in the phasing the supercluster selects (e0 / q0:
// the errtype and callq columns of the original phasing, e1 / q1 of the swapped one), or -1 for a variant that is not counted
// (ERRTYPE_UN etc.: skipped with a warning, print.cpp:374).  *bin: the last of the nq threshold indices the variant counts at,
// nq for one that counts at no threshold (callq < min_qual).
// (the columns come as four pointers: a reference to the kernels' VarCols arguments left all three kernels with scratch)
__device__ __forceinline__ int pr_count_row(int sc, int64_t v, const int32_t *__restrict__ sc_phase, const int32_t *__restrict__ pb_phase,
                                            const uint8_t *e0, const uint8_t *e1, const float *q0, const float *q1,
                                            const uint8_t *__restrict__ cls, int min_qual, int nq, int *bin) {
    const int ph = sc_phase[sc];
    const int swap = ph == VPR_PHASE_ORIG ? 0 : (ph == VPR_PHASE_SWAP ? 1 : (pb_phase ? (pb_phase[sc] != 0) : 0));
    const int e = (swap ? e1 : e0)[v];
    if (e >= 3) return -1;
    const float q = (swap ? q1 : q0)[v];
    int b = (q < float(min_qual)) ? -1 : int(floorf(q)) - min_qual;
    if (b >= nq) b = nq - 1;
    *bin = b < 0 ? nq : b;
    const int t = cls[v] > 2 ? 2 : cls[v];
    return t * 3 + e;
}
