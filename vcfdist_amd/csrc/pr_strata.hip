// pr_strata.hip -- the membership words of the region-stratified counters (include/vcfdist_strata.h): one evaluation, cut by region
// afterwards.  k_strata_mask gives every variant a bit per stratum (the membership rule is the host's vio_bed_contains ==
// VIO_BED_INSIDE, vcf_io.cpp, which follows bedData::contains, bed.cpp:73-121).  What counts behind the words -- k_pr_hist_strata
// and the other cuts -- is pr_cut.hip; its state for the stratified counters lives here, with the words.
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_cut.h"
#include "../../include/vcfdist_strata.h"

struct StrataState {
    int32_t n_strata = 0, n_words = 0;
    int64_t n_var[VPR_HAPS] = {0, 0, 0, 0};
    DevBuf<uint64_t> words[VPR_HAPS];                                   // word-major: [n_words][n_var[slot]]
    bool valid = false;
    // the stratified counters' histogram and device time (ms_strata: vpr_strata_timing's ms_hist); its event pair also times
    // the k_strata_mask launches
    CutState cut;
    double ms_mask = 0;
};

namespace {

const int TYPE_INS = 2;               // VPR_TYPE_INS

}  // namespace

extern "C" {

// One lane per variant, blockIdx.y the 64-stratum word.  The lane walks the word's strata, does the two bisections of
// vio_bed_contains on the stratum's row of its contig and assembles the word in registers: one plain 8-byte store, coalesced
// in the word-major layout.  Consecutive lanes hold consecutive positions of one slot, so the top levels of every
// bisection are wave-uniform and the loads hit the same lines.
__global__ void __launch_bounds__(256) k_strata_mask(const int64_t *__restrict__ var_off, int n_sc, int64_t n_var,
                                                     const int32_t *__restrict__ sc_ctg, const int32_t *__restrict__ var_pos,
                                                     const int32_t *__restrict__ var_ref_len, const uint8_t *__restrict__ var_type,
                                                     const int64_t *__restrict__ iv_off, const int32_t *__restrict__ iv_start,
                                                     const int32_t *__restrict__ iv_stop, int n_strata, int n_ctg,
                                                     uint64_t *__restrict__ words /* [n_words][n_var] */) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n_var) return;
    const int w = blockIdx.y;
    const int ctg = sc_ctg[sc_of_var(var_off, n_sc, v)];
    const int32_t start = var_pos[v], stop = start + var_ref_len[v];
    const bool ins = var_type[v] == TYPE_INS;
    const int k_end = min(n_strata, (w + 1) * 64);
    uint64_t word = 0;
    for (int k = w * 64; k < k_end; k++) {
        const int64_t row = int64_t(k) * n_ctg + ctg;
        const int64_t r0 = iv_off[row];
        const int n = int(iv_off[row + 1] - r0);
        if (n == 0) continue;                                                  // OFFCTG
        const int32_t *__restrict__ st = iv_start + r0, *__restrict__ sp = iv_stop + r0;
        if (stop <= st[0] || start >= sp[n - 1]) continue;                     // OUTSIDE
        int lo = 0, hi = n;              // a = upper_bound(starts, start) - 1
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (st[mid] <= start) lo = mid + 1; else hi = mid; }
        const int a = lo - 1;
        lo = 0; hi = n;                  // b = lower_bound(stops, stop)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (sp[mid] < stop) lo = mid + 1; else hi = mid; }
        const int b = lo;
        // INSIDE: one region holds the whole span, and an insertion does not sit on the region's last base
        if (a >= 0 && b < n && a == b && !(ins && start == sp[b] - 1)) word |= uint64_t(1) << (k & 63);
    }
    words[size_t(w) * size_t(n_var) + size_t(v)] = word;
}

}  // extern "C"

namespace {

void release_words(vpr_handle *h, StrataState *S) {
    for (int s = 0; s < VPR_HAPS; s++) { S->words[s].release(h); S->n_var[s] = 0; }
    S->valid = false;
}

// the state with room for n_words words of n_var[s] variants per slot (earlier words are released)
int strata_prepare(vpr_handle *h, int32_t n_strata, const int64_t n_var[VPR_HAPS]) {
    if (!h->strata) h->strata = new StrataState();
    StrataState *S = h->strata;
    release_words(h, S);
    S->ms_mask = S->cut.ms_strata = 0;
    S->n_strata = n_strata; S->n_words = (n_strata + 63) / 64;
    for (int s = 0; s < VPR_HAPS; s++) {
        const size_t n = std::max<size_t>(size_t(S->n_words) * size_t(n_var[s]), 32);
        if (int rc = S->words[s].reserve(h, n, "stratum membership words: cannot allocate %zu bytes on the device")) {
            release_words(h, S);
            return rc;
        }
        S->n_var[s] = n_var[s];
    }
    return VPR_OK;
}

}  // namespace

void strata_free(vpr_handle *h) {
    StrataState *S = h->strata;
    if (!S) return;
    release_words(h, S);
    cut_release(h, S->cut);
    delete S;
    h->strata = nullptr;
}

// the argument checks of vpr_strata_masks: the interval tables (sorted, non-overlapping, non-empty per row) and the variant
// tables the mask kernel reads (s null: the variant tables alone)
int strata_check(vpr_handle *h, const vpr_variants *v, const vpr_strata *s) {
    if (s) {
        if (s->n_strata < 1) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: n_strata must be at least 1");
        if (s->n_ctg < 1 || s->n_ctg != v->n_ctg)
            return fail(h, VPR_ERR_ARG, "vpr_strata_masks: the strata number %d contigs, the variants %d", s->n_ctg, v->n_ctg);
    }
    if ((s && !s->iv_off) || v->n_sc < 0 || (v->n_sc > 0 && !v->sc_ctg)) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null table");
    if (s) {
        const size_t n_rows = size_t(s->n_strata) * size_t(s->n_ctg);
        if (s->iv_off[0] != 0) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: iv_off[0] is not 0");
        for (size_t r = 0; r < n_rows; r++) {
            const int64_t a = s->iv_off[r], b = s->iv_off[r + 1];
            if (b < a) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: iv_off decreases at row %zu", r);
            if (b > a && (!s->iv_start || !s->iv_stop)) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null interval table");
            if (b - a > INT32_MAX) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: more than 2^31 - 1 intervals in one row");
            const int k = int(r / size_t(s->n_ctg)), c = int(r % size_t(s->n_ctg));
            for (int64_t j = a; j < b; j++) {
                if (s->iv_stop[j] <= s->iv_start[j])
                    return fail(h, VPR_ERR_ARG, "vpr_strata_masks: stratum %d contig %d: region %d-%d has stop <= start", k, c, s->iv_start[j], s->iv_stop[j]);
                if (j > a && s->iv_start[j] < s->iv_start[j - 1])
                    return fail(h, VPR_ERR_ARG, "vpr_strata_masks: stratum %d contig %d is unsorted: region %d-%d precedes %d-%d", k, c,
                                s->iv_start[j - 1], s->iv_stop[j - 1], s->iv_start[j], s->iv_stop[j]);
                if (j > a && s->iv_start[j] < s->iv_stop[j - 1])
                    return fail(h, VPR_ERR_ARG, "vpr_strata_masks: stratum %d contig %d: regions %d-%d and %d-%d overlap", k, c,
                                s->iv_start[j - 1], s->iv_stop[j - 1], s->iv_start[j], s->iv_stop[j]);
            }
        }
    }
    const int64_t n_sc = v->n_sc;
    for (int i = 0; i < VPR_HAPS; i++) {
        if (!v->var_off[i]) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null var_off");
        if (v->var_off[i][n_sc] && (!v->var_pos[i] || !v->var_ref_len[i] || !v->var_type[i])) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null variant column");
    }
    for (int64_t k = 0; k < n_sc; k++)
        if (v->sc_ctg[k] < 0 || v->sc_ctg[k] >= v->n_ctg) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: supercluster %lld names contig %d", (long long)k, v->sc_ctg[k]);
    return VPR_OK;
}

// The membership words of the (checked) variants of `v` against interval tables that are on the device already, in the
// handle's stream order behind whatever filled them: the columns the kernel reads go up in one block that lives as long as
// the call, k_strata_mask runs once per hap slot, and the words are resident when the call returns.
int strata_masks_device(vpr_handle *h, const vpr_variants *v, int32_t n_strata, const int64_t *d_iv_off, const int32_t *d_iv_start,
                        const int32_t *d_iv_stop) {
    const int64_t n_sc = v->n_sc;
    int64_t n_var[VPR_HAPS];
    for (int i = 0; i < VPR_HAPS; i++) n_var[i] = v->var_off[i][n_sc];
    if (int rc = strata_prepare(h, n_strata, n_var)) return rc;
    StrataState *S = h->strata;
    struct Piece { const void *src; size_t bytes; size_t at; };
    std::vector<Piece> pieces;
    size_t total = 0;
    auto add = [&](const void *src, size_t bytes) { pieces.push_back({src, bytes, total}); total += (bytes + 255) & ~size_t(255); return pieces.size() - 1; };
    const size_t i_ctg = add(v->sc_ctg, 4 * size_t(n_sc));
    size_t i_var[VPR_HAPS][4];
    for (int i = 0; i < VPR_HAPS; i++) {
        i_var[i][0] = add(v->var_off[i], 8 * (size_t(n_sc) + 1));
        i_var[i][1] = add(v->var_pos[i], 4 * size_t(n_var[i]));
        i_var[i][2] = add(v->var_ref_len[i], 4 * size_t(n_var[i]));
        i_var[i][3] = add(v->var_type[i], size_t(n_var[i]));
    }
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), std::max<size_t>(total, 256), SITE) != hipSuccess) {
        (void)hipGetLastError();
        release_words(h, S);
        return fail(h, VPR_ERR_NOMEM, "vpr_strata_masks: cannot allocate %zu bytes on the device", total);
    }
    struct Release { vpr_handle *h; uint8_t *p; ~Release() { (void)hipStreamSynchronize(h->stream); (void)x_free(h, p, SITE); } } release{h, blk};
    for (const Piece &p : pieces)
        if (p.bytes && p.src) HIPCHK(h, hipMemcpyAsync(blk + p.at, p.src, p.bytes, hipMemcpyHostToDevice, h->stream));
    auto at = [&](size_t i) { return blk + pieces[i].at; };
    if (int rc = cut_mark(h, S->cut, 0)) return rc;
    for (int i = 0; i < VPR_HAPS; i++) {
        if (!n_var[i]) continue;
        hipLaunchKernelGGL(k_strata_mask, dim3(unsigned((n_var[i] + 255) / 256), unsigned(S->n_words)), dim3(256), 0, h->stream,
                           reinterpret_cast<const int64_t *>(at(i_var[i][0])), int(n_sc), n_var[i], reinterpret_cast<const int32_t *>(at(i_ctg)),
                           reinterpret_cast<const int32_t *>(at(i_var[i][1])), reinterpret_cast<const int32_t *>(at(i_var[i][2])), at(i_var[i][3]),
                           d_iv_off, d_iv_start, d_iv_stop, n_strata, v->n_ctg, S->words[i].p);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = cut_mark(h, S->cut, 1)) return rc;
    HIPCHK(h, x_sync(h, h->stream, SITE));
    S->ms_mask = cut_elapsed(S->cut);
    S->valid = true;
    return VPR_OK;
}

// Room for n_add strata that a kernel of the caller's writes: alone (append false: as strata_prepare, *n_prev = 0) or behind the
// resident ones, whose words are kept (the word-major layout keeps the old words in front; a word array that crosses a 64-bit
// boundary is reallocated and copied).  The words are invalid until strata_commit.
int strata_extend(vpr_handle *h, const char *entry, int32_t n_add, const int64_t n_var[VPR_HAPS], bool append, int32_t *n_prev,
                  uint64_t *words[VPR_HAPS], int32_t *n_words) {
    if (!append) {
        if (int rc = strata_prepare(h, n_add, n_var)) return rc;
        *n_prev = 0;
    } else {
        StrataState *S = h->strata;
        if (!S || !S->valid)
            return fail(h, VPR_ERR_STATE, "%s: append without resident membership words (call vpr_strata_masks, vpr_context_masks or vpr_strata_upload_masks first)", entry);
        for (int s = 0; s < VPR_HAPS; s++)
            if (S->n_var[s] != n_var[s])
                return fail(h, VPR_ERR_STATE, "%s: append: the membership words hold %lld variants of hap slot %d, the variant tables %lld", entry,
                            (long long)S->n_var[s], s, (long long)n_var[s]);
        const int32_t old_words = S->n_words, new_words = (S->n_strata + n_add + 63) / 64;
        S->valid = false;
        for (int s = 0; s < VPR_HAPS; s++) {
            const size_t n = std::max<size_t>(size_t(new_words) * size_t(n_var[s]), 32);
            if (int rc = S->words[s].reserve(h, n, "stratum membership words: cannot allocate %zu bytes on the device", size_t(old_words) * size_t(n_var[s]))) {
                release_words(h, S);
                return rc;
            }
        }
        *n_prev = S->n_strata;
        S->n_strata += n_add; S->n_words = new_words;
    }
    for (int s = 0; s < VPR_HAPS; s++) words[s] = h->strata->words[s].p;
    *n_words = h->strata->n_words;
    return VPR_OK;
}

void strata_commit(vpr_handle *h) { h->strata->valid = true; }

bool strata_resident(const vpr_handle *h, int32_t *n_strata, int64_t n_var[VPR_HAPS]) {
    const StrataState *S = h->strata;
    if (!S || !S->valid) return false;
    *n_strata = S->n_strata;
    for (int s = 0; s < VPR_HAPS; s++) n_var[s] = S->n_var[s];
    return true;
}

CutState &strata_cut(vpr_handle *h) { return h->strata->cut; }

int strata_view(vpr_handle *h, const char *entry, int32_t *n_strata, const uint64_t *words[VPR_HAPS]) {
    const StrataState *S = h->strata;
    if (!S || !S->valid)
        return fail(h, VPR_ERR_STATE, "%s: no membership words (call vpr_strata_masks or vpr_strata_upload_masks after the upload)", entry);
    for (int s = 0; s < VPR_HAPS; s++) {
        if (S->n_var[s] != h->n_var[s])
            return fail(h, VPR_ERR_STATE, "%s: the membership words hold %lld variants of hap slot %d, the executed batch has %lld", entry,
                        (long long)S->n_var[s], s, (long long)h->n_var[s]);
        words[s] = S->words[s].p;
    }
    *n_strata = S->n_strata;
    return VPR_OK;
}

extern "C" {

int vpr_strata_masks(vpr_handle *h, const vpr_variants *v, const vpr_strata *s) {
    if (!h) return VPR_ERR_ARG;
    if (!v || !s) return fail(h, VPR_ERR_ARG, "vpr_strata_masks: null argument");
    if (int rc = strata_check(h, v, s)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // ---- the interval tables: one block that lives as long as the call
    const size_t n_rows = size_t(s->n_strata) * size_t(s->n_ctg), n_iv = size_t(s->iv_off[n_rows]);
    const size_t at_st = (8 * (n_rows + 1) + 255) & ~size_t(255), at_sp = at_st + ((4 * n_iv + 255) & ~size_t(255));
    const size_t total = at_sp + ((4 * n_iv + 255) & ~size_t(255));
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), std::max<size_t>(total, 256), SITE) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, VPR_ERR_NOMEM, "vpr_strata_masks: cannot allocate %zu bytes on the device", total);
    }
    struct Release { vpr_handle *h; uint8_t *p; ~Release() { (void)hipStreamSynchronize(h->stream); (void)x_free(h, p, SITE); } } release{h, blk};
    HIPCHK(h, hipMemcpyAsync(blk, s->iv_off, 8 * (n_rows + 1), hipMemcpyHostToDevice, h->stream));
    if (n_iv) {
        HIPCHK(h, hipMemcpyAsync(blk + at_st, s->iv_start, 4 * n_iv, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(blk + at_sp, s->iv_stop, 4 * n_iv, hipMemcpyHostToDevice, h->stream));
    }
    return strata_masks_device(h, v, s->n_strata, reinterpret_cast<const int64_t *>(blk), reinterpret_cast<const int32_t *>(blk + at_st),
                               reinterpret_cast<const int32_t *>(blk + at_sp));
}

int vpr_strata_timing(const vpr_handle *h, double *ms_mask, double *ms_hist) {
    if (!h || !h->strata || !ms_mask || !ms_hist) return VPR_ERR_ARG;
    *ms_mask = h->strata->ms_mask; *ms_hist = h->strata->cut.ms_strata;
    return VPR_OK;
}

int vpr_strata_download_masks(vpr_handle *h, uint64_t *const mask[VPR_HAPS]) {
    if (!h || !mask) return VPR_ERR_ARG;
    const StrataState *S = h->strata;
    if (!S || !S->valid) return fail(h, VPR_ERR_STATE, "vpr_strata_download_masks: no membership words");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (int s = 0; s < VPR_HAPS; s++) {
        const size_t bytes = size_t(S->n_words) * size_t(S->n_var[s]) * 8;
        if (!bytes) continue;
        if (!mask[s]) return fail(h, VPR_ERR_ARG, "vpr_strata_download_masks: null buffer");
        HIPCHK(h, hipMemcpyAsync(mask[s], S->words[s].p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    return VPR_OK;
}

int vpr_strata_upload_masks(vpr_handle *h, int32_t n_strata, const int64_t n_var[VPR_HAPS], const uint64_t *const mask[VPR_HAPS]) {
    if (!h) return VPR_ERR_ARG;
    if (!n_var || !mask) return fail(h, VPR_ERR_ARG, "vpr_strata_upload_masks: null argument");
    if (n_strata < 1) return fail(h, VPR_ERR_ARG, "vpr_strata_upload_masks: n_strata must be at least 1");
    for (int s = 0; s < VPR_HAPS; s++)
        if (n_var[s] < 0 || (n_var[s] && !mask[s])) return fail(h, VPR_ERR_ARG, "vpr_strata_upload_masks: bad hap slot %d", s);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = strata_prepare(h, n_strata, n_var)) return rc;
    StrataState *S = h->strata;
    for (int s = 0; s < VPR_HAPS; s++) {
        const size_t bytes = size_t(S->n_words) * size_t(n_var[s]) * 8;
        if (bytes) HIPCHK(h, hipMemcpyAsync(S->words[s].p, mask[s], bytes, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    S->valid = true;
    return VPR_OK;
}

}  // extern "C"
