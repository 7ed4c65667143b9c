// Stand-in for htslib's <htslib/kseq.h>: the four names fasta.h uses.  The harness fills fastaData::fasta itself,
// so kseq_read reports end of file at once and the FASTA that Globals::parse_args opened is never tokenised.
#ifndef REF_SHIM_HTSLIB_KSEQ_H
#define REF_SHIM_HTSLIB_KSEQ_H

struct kstring_t { char *s; };
struct kseq_t { kstring_t name, seq; };

#define KSEQ_INIT(type_t, read_fn)                                              \
    static inline kseq_t *kseq_init(type_t) { static kseq_t k; return &k; }     \
    static inline int kseq_read(kseq_t *) { return -1; }                        \
    static inline void kseq_destroy(kseq_t *) {}

#endif
