// pr_varstrata.hip -- the variant strata (include/vcfdist_varstrata.h): strata that are a function of the variant tables alone
// (transition / transversion, insertion and deletion size bins, genotype, crowding).  k_varstrata_mask gives every hap-variant a
// bit per spec entry and writes them into the membership words of pr_strata.hip, alone or behind the resident ones; everything
// behind the words (k_pr_hist_strata, the bootstrap's stratum cut) is the code of pr_strata.hip / pr_cut.hip.
#include "pr_host.h"
#include "pr_counts.h"
#include "pr_varscan.h"
#include "../../include/vcfdist_varstrata.h"

namespace {

const vpr_variant_stratum DEFAULT_SPEC[] = {
    {VPR_VS_TI, 0, 0, 0, 0, 0, 0},
    {VPR_VS_TV, 0, 0, 0, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_INS, 1, 5, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_INS, 6, 15, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_INS, 16, 49, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_INS, 50, 0, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_DEL, 1, 5, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_DEL, 6, 15, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_DEL, 16, 49, 0, 0, 0},
    {VPR_VS_SIZE, VPR_TYPE_DEL, 50, 0, 0, 0, 0},
    {VPR_VS_HOM, 0, 0, 0, 0, 0, 0},
    {VPR_VS_HET, 0, 0, 0, 0, 0, 0},
    {VPR_VS_NEAR, 0, 0, 0, 50, 0, 0},
    {VPR_VS_NEAR, 0, 0, 0, 10, 1, -1},
};
const char *const DEFAULT_NAMES[] = {"snp_ti", "snp_tv", "ins_1to5", "ins_6to15", "ins_16to49", "ins_ge50", "del_1to5", "del_6to15",
                                     "del_16to49", "del_ge50", "hom", "het", "iso_50", "near_10"};

// A, G (the purines) -> 0, 1; C, T (the pyrimidines) -> 2, 3; anything else -1
__device__ __forceinline__ int vs_base(uint8_t b) { return b == 'A' ? 0 : b == 'G' ? 1 : b == 'C' ? 2 : b == 'T' ? 3 : -1; }

}  // namespace

extern "C" {

// One lane per hap-variant of slot `own`; `par` is the partner slot (the other haplotype of the callset).  Consecutive lanes hold
// consecutive positions of one slot, so the top levels of every bisection are wave-uniform and the loads hit the same lines.
// The lane finds its contig's range of both slots (var_off at the contig's first and last supercluster; sc_ctg is non-decreasing),
// counts its copies in the two runs of equal pos (HOM, and the copies N(v) leaves out), takes N(v) of each NEAR entry from two
// bisections per slot, assembles all its spec bits in a register and writes them at bit offset n_prev of the word-major words
// with plain 8-byte stores: a read-modify-write only of the word n_prev falls into, a plain store of the one behind it.
__global__ void __launch_bounds__(256) k_varstrata_mask(VsCols own, VsCols par, int64_t n_var, int n_sc, const int32_t *__restrict__ sc_ctg,
                                                        const vpr_variant_stratum *__restrict__ spec, int n_spec, int n_prev,
                                                        uint64_t *__restrict__ words /* [n_words][n_var] */) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n_var) return;
    const int ctg = sc_ctg[sc_of_var(own.var_off, n_sc, v)];
    int lo = 0, hi = n_sc;               // [c0, c1): the contig's superclusters
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (sc_ctg[mid] < ctg) lo = mid + 1; else hi = mid; }
    const int c0 = lo;
    hi = n_sc;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (sc_ctg[mid] <= ctg) lo = mid + 1; else hi = mid; }
    const int c1 = lo;
    const int64_t o0 = own.var_off[c0], o1 = own.var_off[c1], p0 = par.var_off[c0], p1 = par.var_off[c1];
    const int32_t pos = own.pos[v], ref_len = own.ref_len[v], alt_len = own.alt_len[v];
    const uint8_t type = own.type[v];
    const uint8_t *__restrict__ alt = own.pool + own.alt_off[v];
    const int copies_par = vs_copies(par, p0, p1, -1, pos, type, ref_len, alt_len, alt);
    const int copies_own = vs_copies(own, o0, o1, v, pos, type, ref_len, alt_len, alt);
    bool ti = false, tv = false;
    if (type == VPR_TYPE_SUB && ref_len == 1 && alt_len == 1) {
        const int r = vs_base(own.pool[own.ref_off[v]]), a = vs_base(alt[0]);
        const bool snv = r >= 0 && a >= 0 && r != a;
        ti = snv && (r >> 1) == (a >> 1);
        tv = snv && !ti;
    }
    const int32_t len = type == VPR_TYPE_INS ? alt_len : ref_len;
    int32_t last_w = -1;
    int64_t n_near = 0;
    uint64_t bits = 0;
    for (int k = 0; k < n_spec; k++) {
        const vpr_variant_stratum s = spec[k];
        bool in = false;
        switch (s.kind) {
        case VPR_VS_SIZE: in = type == s.type && len >= s.min_len && (s.max_len == 0 || len <= s.max_len); break;
        case VPR_VS_TI: in = ti; break;
        case VPR_VS_TV: in = tv; break;
        case VPR_VS_HOM: in = copies_par > 0; break;
        case VPR_VS_HET: in = copies_par == 0; break;
        default:       // VPR_VS_NEAR
            if (s.window != last_w) {
                last_w = s.window;
                const int64_t a = int64_t(pos) - s.window, b = int64_t(pos) + s.window;
                n_near = (vs_upper(own.pos, o0, o1, b) - vs_lower(own.pos, o0, o1, a)) + (vs_upper(par.pos, p0, p1, b) - vs_lower(par.pos, p0, p1, a)) -
                       1 - copies_own - copies_par;
            }
            in = n_near >= s.min_n && (s.max_n < 0 || n_near <= s.max_n);
        }
        bits |= uint64_t(in) << k;
    }
    const int w0 = n_prev >> 6, sh = n_prev & 63;
    uint64_t *__restrict__ at = words + size_t(w0) * size_t(n_var) + size_t(v);
    if (sh) {
        *at = (*at & ((uint64_t(1) << sh) - 1)) | (bits << sh);
        if (sh + n_spec > 64) at[n_var] = bits >> (64 - sh);
    } else {
        *at = bits;
    }
}

}  // extern "C"

namespace {

int check_spec(vpr_handle *h, const vpr_variant_stratum *spec, int32_t n_spec) {
    for (int k = 0; k < n_spec; k++) {
        const vpr_variant_stratum &s = spec[k];
        if (s.kind == VPR_VS_SIZE) {
            if (s.type != VPR_TYPE_INS && s.type != VPR_TYPE_DEL)
                return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: type %d is neither VPR_TYPE_INS nor VPR_TYPE_DEL", k, s.type);
            if (s.min_len < 1) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: min_len %d is below 1", k, s.min_len);
            if (s.max_len != 0 && s.max_len < s.min_len)
                return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: max_len %d is neither 0 nor at least min_len %d", k, s.max_len, s.min_len);
        } else if (s.kind == VPR_VS_NEAR) {
            if (s.window < 0) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: window %d is negative", k, s.window);
            if (s.min_n < 0) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: min_n %d is negative", k, s.min_n);
            if (s.max_n != -1 && s.max_n < s.min_n)
                return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: max_n %d is neither -1 nor at least min_n %d", k, s.max_n, s.min_n);
        } else if (s.kind != VPR_VS_TI && s.kind != VPR_VS_TV && s.kind != VPR_VS_HOM && s.kind != VPR_VS_HET) {
            return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: entry %d: unknown kind %d", k, s.kind);
        }
    }
    return VPR_OK;
}

// the variant tables the kernel reads: the preconditions of include/vcfdist_varstrata.h, and per slot the bytes of allele_pool the
// variants name (the pool's extent is not part of vpr_variants)
int check_variants(vpr_handle *h, const vpr_variants *v, size_t pool_len[VPR_HAPS]) {
    const int64_t n_sc = v->n_sc;
    if (n_sc < 0 || (n_sc > 0 && !v->sc_ctg)) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: null table");
    for (int64_t k = 0; k < n_sc; k++) {
        if (v->sc_ctg[k] < 0 || v->sc_ctg[k] >= v->n_ctg)
            return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: supercluster %lld names contig %d", (long long)k, v->sc_ctg[k]);
        if (k > 0 && v->sc_ctg[k] < v->sc_ctg[k - 1])
            return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: sc_ctg decreases at supercluster %lld (contig %d behind contig %d)", (long long)k,
                        v->sc_ctg[k], v->sc_ctg[k - 1]);
    }
    for (int i = 0; i < VPR_HAPS; i++) {
        pool_len[i] = 0;
        const int64_t *off = v->var_off[i];
        if (!off) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: null var_off");
        if (off[0] != 0) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: hap slot %d: var_off[0] is not 0", i);
        for (int64_t k = 0; k < n_sc; k++)
            if (off[k + 1] < off[k]) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: hap slot %d: var_off decreases at supercluster %lld", i, (long long)k);
        if (!off[n_sc]) continue;
        if (!v->var_pos[i] || !v->var_type[i] || !v->var_ref_off[i] || !v->var_ref_len[i] || !v->var_alt_off[i] || !v->var_alt_len[i] || !v->allele_pool[i])
            return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: hap slot %d: null variant column", i);
        int64_t prev = -1;               // the last variant in front, on the same contig
        for (int64_t k = 0; k < n_sc; k++) {
            if (k > 0 && v->sc_ctg[k] != v->sc_ctg[k - 1]) prev = -1;
            for (int64_t j = off[k]; j < off[k + 1]; j++) {
                if (prev >= 0 && v->var_pos[i][j] < v->var_pos[i][prev])
                    return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: hap slot %d: var_pos is unsorted: variant %lld at %d follows one at %d on contig %d", i,
                                (long long)j, v->var_pos[i][j], v->var_pos[i][prev], v->sc_ctg[k]);
                prev = j;
                const int64_t ro = v->var_ref_off[i][j], ao = v->var_alt_off[i][j];
                const int32_t rl = v->var_ref_len[i][j], al = v->var_alt_len[i][j];
                if (ro < 0 || ao < 0 || rl < 0 || al < 0)
                    return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: hap slot %d: variant %lld has a negative allele offset or length", i, (long long)j);
                pool_len[i] = std::max(pool_len[i], std::max(size_t(ro) + size_t(rl), size_t(ao) + size_t(al)));
            }
        }
    }
    return VPR_OK;
}

}  // namespace

extern "C" {

int vpr_varstrata_default(const vpr_variant_stratum **spec, const char *const **names, int32_t *n) {
    if (!spec || !names || !n) return VPR_ERR_ARG;
    *spec = DEFAULT_SPEC; *names = DEFAULT_NAMES; *n = int32_t(sizeof(DEFAULT_SPEC) / sizeof(DEFAULT_SPEC[0]));
    return VPR_OK;
}

int vpr_varstrata_masks(vpr_handle *h, const vpr_variants *v, const vpr_variant_stratum *spec, int32_t n_spec, int32_t append) {
    if (!h) return VPR_ERR_ARG;
    if (!v || !spec) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: null argument");
    if (n_spec < 1 || n_spec > VPR_VS_MAX_SPEC) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: n_spec %d is not in 1..%d", n_spec, VPR_VS_MAX_SPEC);
    if (append != 0 && append != 1) return fail(h, VPR_ERR_ARG, "vpr_varstrata_masks: append %d is neither 0 nor 1", append);
    if (int rc = check_spec(h, spec, n_spec)) return rc;
    size_t pool_len[VPR_HAPS];
    if (int rc = check_variants(h, v, pool_len)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->varstrata_ms = 0;
    const int64_t n_sc = v->n_sc;
    int64_t n_var[VPR_HAPS];
    for (int i = 0; i < VPR_HAPS; i++) n_var[i] = v->var_off[i][n_sc];
    // ---- the columns, the pools and the spec: one block that lives as long as the call
    struct Piece { const void *src; size_t bytes; size_t at; };
    std::vector<Piece> pieces;
    size_t total = 0;
    auto add = [&](const void *src, size_t bytes) { pieces.push_back({src, bytes, total}); total += (bytes + 255) & ~size_t(255); return pieces.size() - 1; };
    const size_t i_ctg = add(v->sc_ctg, 4 * size_t(n_sc)), i_spec = add(spec, sizeof(vpr_variant_stratum) * size_t(n_spec));
    size_t i_var[VPR_HAPS][8];
    for (int i = 0; i < VPR_HAPS; i++) {
        const size_t n = size_t(n_var[i]);
        i_var[i][0] = add(v->var_off[i], 8 * (size_t(n_sc) + 1));
        i_var[i][1] = add(v->var_ref_off[i], 8 * n);
        i_var[i][2] = add(v->var_alt_off[i], 8 * n);
        i_var[i][3] = add(v->var_pos[i], 4 * n);
        i_var[i][4] = add(v->var_ref_len[i], 4 * n);
        i_var[i][5] = add(v->var_alt_len[i], 4 * n);
        i_var[i][6] = add(v->var_type[i], n);
        i_var[i][7] = add(v->allele_pool[i], n ? pool_len[i] : 0);
    }
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), std::max<size_t>(total, 256), SITE) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, VPR_ERR_NOMEM, "vpr_varstrata_masks: cannot allocate %zu bytes on the device", total);
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
    if (int rc = strata_extend(h, "vpr_varstrata_masks", n_spec, n_var, append != 0, &n_prev, words, &n_words)) return rc;
    for (const Piece &p : pieces)
        if (p.bytes && p.src) HIPCHK(h, hipMemcpyAsync(blk + p.at, p.src, p.bytes, hipMemcpyHostToDevice, h->stream));
    auto at = [&](size_t i) { return blk + pieces[i].at; };
    VsCols cols[VPR_HAPS];
    for (int i = 0; i < VPR_HAPS; i++)
        cols[i] = VsCols{reinterpret_cast<const int64_t *>(at(i_var[i][0])), reinterpret_cast<const int64_t *>(at(i_var[i][1])),
                         reinterpret_cast<const int64_t *>(at(i_var[i][2])), reinterpret_cast<const int32_t *>(at(i_var[i][3])),
                         reinterpret_cast<const int32_t *>(at(i_var[i][4])), reinterpret_cast<const int32_t *>(at(i_var[i][5])),
                         at(i_var[i][6]), at(i_var[i][7])};
    HIPCHK(h, hipEventRecord(R.ev[0], h->stream));
    for (int i = 0; i < VPR_HAPS; i++) {
        if (!n_var[i]) continue;
        hipLaunchKernelGGL(k_varstrata_mask, dim3(unsigned((n_var[i] + 255) / 256)), dim3(256), 0, h->stream, cols[i], cols[i ^ 1], n_var[i], int(n_sc),
                           reinterpret_cast<const int32_t *>(at(i_ctg)), reinterpret_cast<const vpr_variant_stratum *>(at(i_spec)), int(n_spec),
                           int(n_prev), words[i]);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(R.ev[1], h->stream));
    HIPCHK(h, x_sync(h, h->stream, SITE));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, R.ev[0], R.ev[1]);
    h->varstrata_ms = ms;
    strata_commit(h);
    return VPR_OK;
}

int vpr_varstrata_timing(const vpr_handle *h, double *ms_mask) {
    if (!h || !ms_mask) return VPR_ERR_ARG;
    *ms_mask = h->varstrata_ms;
    return VPR_OK;
}

}  // extern "C"
