// pr_bootw.h -- what the two replicate kernels (k_pr_boot, pr_boot.hip: the counters; k_label_boot, pr_labelcut.hip: the label
// counts) decide alike: the weight w(seed, replicate, key) of include/vcfdist_bootstrap.h with its table, and the launch shape of
// a [bin][64 replicates] LDS table -- the LDS budget, the waves of a workgroup and the variant spans.
#pragma once

#include "pr_host.h"
#include "../../include/vcfdist_bootstrap.h"

namespace {

// LDS a workgroup may ask for: one workgroup per compute unit (160 KiB), with room left for 64 quality bins a slice
// (9 x 64 x 64 x 4 B = 144 KiB; -mn 0 -mx 60 needs 62)
const size_t BOOT_LDS_BUDGET = 144 * 1024;
// waves of a workgroup (VPR_BOOT_WAVES: 4 .. 16).  Measured on 2 993 023 hap-variants x 1 000 replicates: 4 waves 12.3 ms,
// 8 waves 7.0 ms, 16 waves 5.2 ms (profiles/boot_bench.json): the table admits one workgroup a compute unit, so its waves
// are all the latency hiding there is
const int BOOT_WAVES = 16;
const int64_t BOOT_SPAN_MIN = 1024;               // a slot of 2 048 variants or more runs in at least two spans
const int64_t BOOT_SPAN_MAX = int64_t(1) << 24;   // x 12 < 2^32: a uint32 bin of the table cannot wrap
// workgroups of a launch from which spans stop getting shorter (VPR_BOOT_WG_TARGET).  Measured as above at 16 waves:
// 256 workgroups 4.84 ms, 512 4.86 ms, 1 024 4.95 ms, 2 048 5.18 ms, 4 096 5.93 ms, 16 384 7.50 ms -- every workgroup zeroes
// and flushes a whole table.  512 is two rounds over the 256 compute units: within 1 % of one round, less of a tail
const int64_t BOOT_WG_TARGET = 512;

__device__ const uint32_t BOOT_T[VPR_BOOT_MAX_WEIGHT] = VPR_BOOT_T;

// w(seed, r, key): `salt` is the lane's 0x9E3779B97F4A7C15 * (r + 1) + seed * 0xD1B54A32D192ED03
__device__ inline uint32_t boot_weight(uint64_t key, uint64_t salt) {
    uint64_t z = key + salt;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const uint32_t u = uint32_t(z >> 32);
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < VPR_BOOT_MAX_WEIGHT; k++) w += u >= BOOT_T[k];
    return w;
}

inline int boot_waves() {
    int n = BOOT_WAVES;
    if (const char *e = getenv("VPR_BOOT_WAVES")) n = atoi(e);      // diagnostic
    return std::max(4, std::min(16, n));
}

// variants of a span of a slot of nv variants, in a launch whose other grid dimensions multiply to `others`
inline int64_t boot_span(int64_t nv, int64_t others) {
    int64_t target = BOOT_WG_TARGET;
    if (const char *e = getenv("VPR_BOOT_WG_TARGET")) target = std::max(1, atoi(e));      // diagnostic
    const int64_t want = std::max<int64_t>(2, (target + others - 1) / others);
    int64_t span = std::max(BOOT_SPAN_MIN, (nv + want - 1) / want);
    span = (span + 63) & ~int64_t(63);
    return std::min(span, BOOT_SPAN_MAX);
}

}  // namespace
