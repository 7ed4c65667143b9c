// pr_derive.hip -- the derived strata (include/vcfdist_derive.h): boolean combinations of the strata that are there.  k_derive_mask
// runs a postfix program per new stratum over every hap-variant's resident membership bits and appends the results to the words of
// pr_strata.hip; everything behind the words (k_pr_hist_strata, the bootstrap's stratum cut, the label cuts) is the code of
// pr_cut.hip.  The text in front of the programs (NAME=EXPR, LIST:LIST) is compiled on the host: derive.cpp.
#include "pr_host.h"
#include "../../include/vcfdist_derive.h"

extern "C" {

// One lane per hap-variant of a slot.  The code is the same for every lane: it is read through a pointer nothing is written
// through, at indices made of kernel arguments and loop counters, so the loads are scalar and the branches on an opcode are
// wave-uniform -- the lanes differ in their bits alone.  The stack is a 32-bit register, bit 0 its top: a push shifts one bit in.
// The new strata are assembled one 64-bit word at a time in `acc`; the first word starts as the old one masked to its n_prev & 63
// low bits and is stored over it (the read-modify-write of k_varstrata_mask), later words are plain stores.  An operand in the word
// being assembled is read from `acc`; any other from words[(c >> 6) * n_var + v] -- coalesced, c being wave-uniform -- through a
// one-word cache.  A cached word cannot go stale: it is either an old word in front of the first output word, which no one
// writes, or an output word this lane has finished and stored itself.  No lane reads another lane's store.
__global__ void __launch_bounds__(256) k_derive_mask(const int32_t *__restrict__ code_off /* [n_entries + 1] */, const int32_t *__restrict__ code,
                                                     int n_entries, int n_prev, int64_t n_var, uint64_t *words /* [n_words][n_var] */) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n_var) return;
    uint64_t *at = words + size_t(v);
    int cur_w = n_prev >> 6;                              // the word being assembled
    const int sh = n_prev & 63;
    uint64_t acc = sh ? at[size_t(cur_w) * size_t(n_var)] & ((uint64_t(1) << sh) - 1) : 0;
    int cache_w = -1;
    uint64_t cache = 0;
    for (int j = 0; j < n_entries; j++) {
        const int k = n_prev + j;
        if ((k >> 6) != cur_w) {
            at[size_t(cur_w) * size_t(n_var)] = acc;
            cur_w = k >> 6; acc = 0;
        }
        uint32_t st = 0;
        const int end = code_off[j + 1];
        for (int i = code_off[j]; i < end; i++) {
            const int c = code[i];
            if (c >= 0) {
                const int w = c >> 6;
                uint64_t word = acc;
                if (w != cur_w) {
                    if (w != cache_w) { cache = at[size_t(w) * size_t(n_var)]; cache_w = w; }
                    word = cache;
                }
                st = (st << 1) | uint32_t((word >> (c & 63)) & 1);
            } else if (c == VPR_DV_AND) {
                st = (st >> 1) & (st | ~uint32_t(1));
            } else if (c == VPR_DV_OR) {
                st = (st >> 1) | (st & 1);
            } else {                                      // VPR_DV_NOT
                st ^= 1;
            }
        }
        acc |= uint64_t(st & 1) << (k & 63);
    }
    at[size_t(cur_w) * size_t(n_var)] = acc;
}

}  // extern "C"

namespace {

// the programs against the definition of include/vcfdist_derive.h; entry j may name the strata in front of n_prev + j
int check_programs(vpr_handle *h, const int32_t *code_off, const int32_t *code, int32_t n_entries, int32_t n_prev) {
    if (code_off[0] != 0) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: code_off[0] is not 0");
    for (int32_t j = 0; j < n_entries; j++) {
        if (code_off[j + 1] < code_off[j]) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: code_off decreases", j);
        if (code_off[j + 1] > VPR_DV_MAX_CODE)
            return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: the code of the call exceeds %d ints", j, VPR_DV_MAX_CODE);
        int depth = 0;
        for (int32_t i = code_off[j]; i < code_off[j + 1]; i++) {
            const int32_t c = code[i];
            if (c >= 0) {
                if (c >= n_prev + j)
                    return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: operand %d at code %d is not a stratum in front of stratum %d", j, c, i - code_off[j],
                                n_prev + j);
                if (++depth > VPR_DV_MAX_DEPTH)
                    return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: the stack exceeds %d at code %d", j, VPR_DV_MAX_DEPTH, i - code_off[j]);
            } else if (c == VPR_DV_AND || c == VPR_DV_OR) {
                if (depth < 2) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: the stack underflows at code %d", j, i - code_off[j]);
                depth--;
            } else if (c == VPR_DV_NOT) {
                if (depth < 1) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: the stack underflows at code %d", j, i - code_off[j]);
            } else {
                return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: unknown opcode %d at code %d", j, c, i - code_off[j]);
            }
        }
        if (depth != 1) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: entry %d: the stack ends at depth %d, not 1", j, depth);
    }
    return VPR_OK;
}

}  // namespace

extern "C" {

int vpr_derive_masks(vpr_handle *h, const int32_t *code_off, const int32_t *code, int32_t n_entries) {
    if (!h) return VPR_ERR_ARG;
    if (!code_off || !code) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: null argument");
    if (n_entries < 1 || n_entries > VPR_DV_MAX_SPEC) return fail(h, VPR_ERR_ARG, "vpr_derive_masks: n_entries %d is not in 1..%d", n_entries, VPR_DV_MAX_SPEC);
    int32_t n_old = 0;
    int64_t n_var[VPR_HAPS];
    if (!strata_resident(h, &n_old, n_var))
        return fail(h, VPR_ERR_STATE, "vpr_derive_masks: no resident membership words (call vpr_strata_masks, vpr_context_masks, vpr_varstrata_masks or "
                                      "vpr_strata_upload_masks first)");
    if (int rc = check_programs(h, code_off, code, n_entries, n_old)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->derive_ms = 0;
    // ---- the code: one block that lives as long as the call
    const size_t n_code = size_t(code_off[n_entries]);
    const size_t at_code = (4 * (size_t(n_entries) + 1) + 255) & ~size_t(255), total = at_code + ((4 * n_code + 255) & ~size_t(255));
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), total, SITE) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, VPR_ERR_NOMEM, "vpr_derive_masks: cannot allocate %zu bytes on the device", total);
    }
    struct Release {
        vpr_handle *h; uint8_t *p; hipEvent_t ev[2];
        ~Release() {
            (void)hipStreamSynchronize(h->stream);
            (void)x_free(h, p, SITE);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        }
    } R{h, blk, {nullptr, nullptr}};
    for (int k = 0; k < 2; k++) HIPCHK(h, hipEventCreate(&R.ev[k]));
    int32_t n_prev = 0, n_words = 0;
    uint64_t *words[VPR_HAPS];
    if (int rc = strata_extend(h, "vpr_derive_masks", n_entries, n_var, true, &n_prev, words, &n_words)) return rc;
    HIPCHK(h, hipMemcpyAsync(blk, code_off, 4 * (size_t(n_entries) + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(blk + at_code, code, 4 * n_code, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(R.ev[0], h->stream));
    for (int i = 0; i < VPR_HAPS; i++) {
        if (!n_var[i]) continue;
        hipLaunchKernelGGL(k_derive_mask, dim3(unsigned((n_var[i] + 255) / 256)), dim3(256), 0, h->stream, reinterpret_cast<const int32_t *>(blk),
                           reinterpret_cast<const int32_t *>(blk + at_code), int(n_entries), int(n_prev), n_var[i], words[i]);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(R.ev[1], h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, R.ev[0], R.ev[1]);
    h->derive_ms = ms;
    strata_commit(h);
    return VPR_OK;
}

int vpr_derive_timing(const vpr_handle *h, double *ms_mask) {
    if (!h || !ms_mask) return VPR_ERR_ARG;
    *ms_mask = h->derive_ms;
    return VPR_OK;
}

}  // extern "C"
