// pr_vartab.hip -- the host check and the one-block upload of the variant tables (pr_vartab.h) for the entries that join the two
// callsets inside a supercluster: vpr_errclass and vpr_matchkind.
#include "pr_vartab.h"

VarTables::~VarTables() {
    if (!blk) return;
    (void)hipStreamSynchronize(h->stream);
    (void)x_free(h, blk, SITE);
}

int vartab_check(vpr_handle *h, const char *entry, const vpr_variants *v, size_t pool_len[VPR_HAPS]) {
    if (v->n_sc != h->n_sc)
        return fail(h, VPR_ERR_STATE, "%s: the variant tables hold %d superclusters, the resident batch %d", entry, v->n_sc, h->n_sc);
    const int64_t n_sc = v->n_sc;
    for (int i = 0; i < VPR_HAPS; i++) {
        pool_len[i] = 0;
        const int64_t *off = v->var_off[i];
        if (!off) return fail(h, VPR_ERR_ARG, "%s: null var_off", entry);
        if (off[0] != 0) return fail(h, VPR_ERR_ARG, "%s: hap slot %d: var_off[0] is not 0", entry, i);
        for (int64_t k = 0; k < n_sc; k++)
            if (off[k + 1] < off[k]) return fail(h, VPR_ERR_ARG, "%s: hap slot %d: var_off decreases at supercluster %lld", entry, i, (long long)k);
        if (off[n_sc] != h->n_var[i])
            return fail(h, VPR_ERR_STATE, "%s: hap slot %d: the variant tables hold %lld variants, the resident batch %lld", entry, i,
                        (long long)off[n_sc], (long long)h->n_var[i]);
        if (!off[n_sc]) continue;
        if (!v->var_pos[i] || !v->var_type[i] || !v->var_ref_len[i] || !v->var_alt_off[i] || !v->var_alt_len[i] || !v->allele_pool[i])
            return fail(h, VPR_ERR_ARG, "%s: hap slot %d: null variant column", entry, i);
        for (int64_t k = 0; k < n_sc; k++)
            for (int64_t j = off[k]; j < off[k + 1]; j++) {
                if (j > off[k] && v->var_pos[i][j] < v->var_pos[i][j - 1])
                    return fail(h, VPR_ERR_ARG, "%s: hap slot %d: var_pos is unsorted inside supercluster %lld: variant %lld at %d follows one at %d",
                                entry, i, (long long)k, (long long)j, v->var_pos[i][j], v->var_pos[i][j - 1]);
                const int64_t ao = v->var_alt_off[i][j];
                const int32_t rl = v->var_ref_len[i][j], al = v->var_alt_len[i][j];
                if (ao < 0 || rl < 0 || al < 0)
                    return fail(h, VPR_ERR_ARG, "%s: hap slot %d: variant %lld has a negative allele offset or length", entry, i, (long long)j);
                pool_len[i] = std::max(pool_len[i], size_t(ao) + size_t(al));
            }
    }
    return VPR_OK;
}

int vartab_upload(vpr_handle *h, const char *entry, const vpr_variants *v, const size_t pool_len[VPR_HAPS], VarTables *T) {
    struct Piece { const void *src; size_t bytes; size_t at; };
    std::vector<Piece> pieces;
    size_t total = 0;
    auto add = [&](const void *src, size_t bytes) { pieces.push_back({src, bytes, total}); total += (bytes + 255) & ~size_t(255); return pieces.size() - 1; };
    const int64_t n_sc = v->n_sc;
    size_t i_var[VPR_HAPS][7];
    for (int i = 0; i < VPR_HAPS; i++) {
        const size_t n = size_t(h->n_var[i]);
        i_var[i][0] = add(v->var_off[i], 8 * (size_t(n_sc) + 1));
        i_var[i][1] = add(v->var_alt_off[i], 8 * n);
        i_var[i][2] = add(v->var_pos[i], 4 * n);
        i_var[i][3] = add(v->var_ref_len[i], 4 * n);
        i_var[i][4] = add(v->var_alt_len[i], 4 * n);
        i_var[i][5] = add(v->var_type[i], n);
        i_var[i][6] = add(v->allele_pool[i], n ? pool_len[i] : 0);
    }
    uint8_t *blk = nullptr;
    if (x_malloc(h, reinterpret_cast<void **>(&blk), std::max<size_t>(total, 256), SITE) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, VPR_ERR_NOMEM, "%s: cannot allocate %zu bytes on the device", entry, total);
    }
    T->h = h; T->blk = blk;
    for (const Piece &p : pieces)
        if (p.bytes && p.src) HIPCHK(h, hipMemcpyAsync(blk + p.at, p.src, p.bytes, hipMemcpyHostToDevice, h->stream));
    auto at = [&](size_t i) { return blk + pieces[i].at; };
    for (int i = 0; i < VPR_HAPS; i++)
        T->cols[i] = VsCols{reinterpret_cast<const int64_t *>(at(i_var[i][0])), nullptr, reinterpret_cast<const int64_t *>(at(i_var[i][1])),
                            reinterpret_cast<const int32_t *>(at(i_var[i][2])), reinterpret_cast<const int32_t *>(at(i_var[i][3])),
                            reinterpret_cast<const int32_t *>(at(i_var[i][4])), at(i_var[i][5]), at(i_var[i][6])};
    return VPR_OK;
}
