// pr_ctxdev.h -- device helpers shared by the kernels that walk the concatenated contig sequences: pr_context.hip (the context
// strata's flag and run kernels), pr_repeats.hip (the pack and mark kernels) and pr_longrepeats.hip (the pair and valid kernels).
#ifndef PR_CTXDEV_H_
#define PR_CTXDEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ inline bool called(unsigned x) { return x == 'A' || x == 'C' || x == 'G' || x == 'T'; }

// contig of base G of the concatenation (0 <= G < ctg_off[n_ctg]): the largest c with ctg_off[c] <= G, which is not empty
__device__ inline int ctg_of(const int64_t *__restrict__ ctg_off, int n_ctg, int64_t G) {
    int lo = 0, hi = n_ctg;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ctg_off[mid] <= G) lo = mid; else hi = mid; }
    return lo;
}

// exclusive prefix sum of one value per lane over a workgroup of 256; *total: the workgroup's sum
__device__ inline uint32_t block_scan(uint32_t v, uint32_t *lds /* [4] */, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t s = lds[k]; if (k < wave) before += s; all += s; }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

}  // namespace

#endif
