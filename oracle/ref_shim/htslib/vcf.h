// Stand-in for htslib's <htslib/vcf.h>, written for oracle/ref_harness.cpp: only the names that vcfdist's sources
// mention, declared so that those sources compile unmodified.  Nothing here reads a VCF; the definitions
// (../shim.cpp) abort when called, except bcf_open / bcf_close.  Field and function names follow the public
// htslib API; the layouts are ours and hold only the members that are used.
#ifndef REF_SHIM_HTSLIB_VCF_H
#define REF_SHIM_HTSLIB_VCF_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" {

struct htsFile { int dummy; };
typedef htsFile vcfFile;

enum { BCF_HL_FLT = 0, BCF_HL_INFO = 1, BCF_HL_FMT = 2, BCF_HL_CTG = 3, BCF_HL_STR = 4, BCF_HL_GEN = 5 };
enum { BCF_UN_STR = 1, BCF_UN_FLT = 2, BCF_UN_INFO = 4, BCF_UN_SHR = 7, BCF_UN_FMT = 8, BCF_UN_ALL = 15 };

struct bcf_hrec_t {
    int type;
    char *key, *value;
    int nkeys;
    char **keys, **vals;
};

struct bcf_hdr_t {
    int nhrec;
    bcf_hrec_t **hrec;
    char **samples;
    int nsamples;
};

struct bcf_dec_t {
    int n_flt;
    int *flt;
    char **allele;
};

struct bcf1_t {
    int64_t pos, rlen;
    int32_t rid;
    float qual;
    uint32_t n_allele;
    bcf_dec_t d;
};

htsFile *bcf_open(const char *fn, const char *mode);
int bcf_close(htsFile *fp);
bcf_hdr_t *bcf_hdr_read(htsFile *fp);
void bcf_hdr_destroy(bcf_hdr_t *h);
int bcf_hdr_nsamples(const bcf_hdr_t *h);
const char **bcf_hdr_seqnames(const bcf_hdr_t *h, int *nseqs);
bcf1_t *bcf_init(void);
void bcf_destroy(bcf1_t *v);
int bcf_read(htsFile *fp, const bcf_hdr_t *h, bcf1_t *v);
int bcf_unpack(bcf1_t *v, int which);
int bcf_get_format_int32(const bcf_hdr_t *h, bcf1_t *v, const char *tag, int32_t **dst, int *ndst);
int bcf_get_format_float(const bcf_hdr_t *h, bcf1_t *v, const char *tag, float **dst, int *ndst);

// genotype words: (allele + 1) << 1 | phased, 0 for a missing allele
static inline int bcf_gt_is_missing(int v) { return (v >> 1) == 0; }
static inline int bcf_gt_is_phased(int v) { return v & 1; }
static inline int bcf_gt_allele(int v) { return (v >> 1) - 1; }

}  // extern "C"

#endif
