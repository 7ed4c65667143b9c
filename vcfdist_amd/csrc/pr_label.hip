// pr_label.hip -- the host side of a label pass (pr_label.h): the front and the back of a call around the pass's own launches, the
// fold of the label histogram, the download of the label bytes, the device time and the release with the batch.  The front and back
// of a counters call are the ones of pr_collect.hip; the check and the upload of the variant tables are pr_vartab.h's.
#include "pr_label.h"

int label_begin(vpr_handle *h, const LabelDesc &D, void *comm, const vpr_variants *v, const uint8_t *const var_class[VPR_HAPS],
                const int32_t *pb_phase, int32_t min_qual, int32_t max_qual, const int64_t *counts, LabelCall *c) {
    if (!v || !counts) return fail(h, VPR_ERR_ARG, "%s: null argument", D.entry);
    if (max_qual < min_qual) return fail(h, VPR_ERR_ARG, "%s: max_qual %d is below min_qual %d", D.entry, max_qual, min_qual);
    if (int64_t(max_qual) - min_qual >= label_max_nq(D))
        return fail(h, VPR_ERR_ARG, "%s: the quality range %d..%d holds more than %d thresholds (the block histogram is in LDS)", D.entry, min_qual,
                    max_qual, label_max_nq(D));
    if (int rc = pr_counts_begin(h, D.entry, comm)) return rc;
    size_t pool_len[VPR_HAPS];
    if (int rc = vartab_check(h, D.entry, v, pool_len)) return rc;
    if (!h->label[D.pass]) h->label[D.pass] = new LabelState();
    LabelState *S = c->S = h->label[D.pass];
    S->valid = false; S->ms = 0;
    for (int k = 0; k < 2; k++) if (!S->ev[k]) HIPCHK(h, hipEventCreate(&S->ev[k]));
    c->nq = max_qual - min_qual + 1;
    c->nb = size_t(3) * D.labels * size_t(c->nq + 1);
    char nomem[2][128];      // DevBuf::reserve's formats, one %zu each
    snprintf(nomem[0], sizeof(nomem[0]), "%s: %s bytes: cannot allocate %%zu bytes on the device", D.entry, D.noun);
    snprintf(nomem[1], sizeof(nomem[1]), "%s: %s histogram: cannot allocate %%zu bytes on the device", D.entry, D.noun);
    for (int i = 0; i < VPR_HAPS; i++)
        if (int rc = S->bytes[i].reserve(h, size_t(h->n_var[i]), nomem[0])) return rc;
    if (int rc = S->hist.reserve(h, 2 * c->nb, nomem[1])) return rc;
    if (int rc = vartab_upload(h, D.entry, v, pool_len, &c->T)) return rc;
    HIPCHK(h, hipMemsetAsync(S->hist.p, 0, 2 * c->nb * 8, h->stream));
    if (int rc = pr_counts_inputs(h, D.entry, var_class, pb_phase, &c->d_pb)) return rc;
    S->has_pb = c->d_pb != nullptr;      // the cuts' copy of the phasing of this call (h->d_pb is the next counters call's)
    if (S->has_pb) {
        char nomem_pb[128];
        snprintf(nomem_pb, sizeof(nomem_pb), "%s: phase-block phasing: cannot allocate %%zu bytes on the device", D.entry);
        if (int rc = S->pb.reserve(h, size_t(h->n_sc), nomem_pb)) return rc;
        HIPCHK(h, hipMemcpyAsync(S->pb.p, c->d_pb, size_t(h->n_sc) * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipEventRecord(S->ev[0], h->stream));
    return VPR_OK;
}

int label_finish(vpr_handle *h, const LabelDesc &D, void *comm, LabelCall *c, int64_t *counts) {
    LabelState *S = c->S;
    HIPCHK(h, hipEventRecord(S->ev[1], h->stream));
    std::vector<unsigned long long> hist(2 * c->nb);
    if (int rc = pr_counts_finish(h, comm, S->hist.p, hist.size(), hist.data())) return rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]);
    S->ms = ms; S->valid = true;
    fold_labels(D, hist.data(), c->nq, counts);
    return VPR_OK;
}

void fold_labels(const LabelDesc &D, const unsigned long long *hist, int nq, int64_t *counts) {
    const size_t L = size_t(D.labels);
    std::fill(counts, counts + size_t(2) * VPR_VARTYPES * L * size_t(nq), 0);
    auto C = [&](int cs, int t, int c, int k) -> int64_t & { return counts[((size_t(cs) * VPR_VARTYPES + t) * L + c) * nq + k]; };
    for (int cs = 0; cs < 2; cs++)
        for (int t = 0; t < 3; t++)
            for (int c = 0; c < D.labels; c++) {
                const unsigned long long *b = hist + ((size_t(cs) * 3 + t) * L + c) * (nq + 1);
                int64_t acc = 0;
                switch (D.fold(cs, c)) {
                case LABEL_FOLD_UPTO:
                    for (int k = nq - 1; k >= 0; k--) { acc += int64_t(b[k]); C(cs, t, c, k) = acc; }
                    break;
                case LABEL_FOLD_EVERY:
                    for (int k = 0; k <= nq; k++) acc += int64_t(b[k]);
                    for (int k = 0; k < nq; k++) C(cs, t, c, k) = acc;
                    break;
                case LABEL_FOLD_ABOVE:
                    acc = int64_t(b[nq]);
                    for (int k = 0; k < nq; k++) { C(cs, t, c, k) = acc; acc += int64_t(b[k]); }
                    break;
                }
                for (int k = 0; k < nq; k++) C(cs, VPR_VARTYPE_ALL, c, k) += C(cs, t, c, k);
            }
}

int label_download(vpr_handle *h, const LabelDesc &D, uint8_t *const bytes[VPR_HAPS]) {
    if (!h || !bytes) return VPR_ERR_ARG;
    const LabelState *S = h->label[D.pass];
    if (!S || !S->valid)
        return fail(h, VPR_ERR_STATE, "%s_download: no %s bytes (before %s, or after the next upload)", D.entry, D.noun, D.entry);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (int s = 0; s < VPR_HAPS; s++) {
        if (!h->n_var[s]) continue;
        if (!bytes[s]) return fail(h, VPR_ERR_ARG, "%s_download: hap slot %d: null array", D.entry, s);
        HIPCHK(h, hipMemcpyAsync(bytes[s], S->bytes[s].p, size_t(h->n_var[s]), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, x_sync(h, h->stream, SITE));
    return VPR_OK;
}

int label_timing(const vpr_handle *h, const LabelDesc &D, double *ms) {
    if (!h || !ms) return VPR_ERR_ARG;
    *ms = h->label[D.pass] ? h->label[D.pass]->ms : 0;
    return VPR_OK;
}

void label_free(vpr_handle *h) {
    for (LabelState *&S : h->label) {
        if (!S) continue;
        dev_release(h, S->bytes[0], S->bytes[1], S->bytes[2], S->bytes[3], S->hist, S->pb);
        for (int k = 0; k < 2; k++) if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
        cut_release(h, S->cut);
        delete S;
        S = nullptr;
    }
}
