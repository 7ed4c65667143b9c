// Definitions behind ref_shim/htslib/vcf.h.  The harness never reads a VCF: every function says its name and
// aborts, except bcf_open / bcf_close, which hand out a dummy handle so that Globals::parse_args (which only opens
// and closes the two VCFs) fills the reference's globals from a real argument list.
#include "htslib/vcf.h"

#define REF_SHIM_TRAP(name) do { fprintf(stderr, "ref_shim: %s called, but the harness has no VCF reader\n", name); abort(); } while (0)

extern "C" {

static htsFile g_dummy;

htsFile *bcf_open(const char *, const char *) { return &g_dummy; }
int bcf_close(htsFile *) { return 0; }
bcf_hdr_t *bcf_hdr_read(htsFile *) { REF_SHIM_TRAP("bcf_hdr_read"); }
void bcf_hdr_destroy(bcf_hdr_t *) { REF_SHIM_TRAP("bcf_hdr_destroy"); }
int bcf_hdr_nsamples(const bcf_hdr_t *) { REF_SHIM_TRAP("bcf_hdr_nsamples"); }
const char **bcf_hdr_seqnames(const bcf_hdr_t *, int *) { REF_SHIM_TRAP("bcf_hdr_seqnames"); }
bcf1_t *bcf_init(void) { REF_SHIM_TRAP("bcf_init"); }
void bcf_destroy(bcf1_t *) { REF_SHIM_TRAP("bcf_destroy"); }
int bcf_read(htsFile *, const bcf_hdr_t *, bcf1_t *) { REF_SHIM_TRAP("bcf_read"); }
int bcf_unpack(bcf1_t *, int) { REF_SHIM_TRAP("bcf_unpack"); }
int bcf_get_format_int32(const bcf_hdr_t *, bcf1_t *, const char *, int32_t **, int *) { REF_SHIM_TRAP("bcf_get_format_int32"); }
int bcf_get_format_float(const bcf_hdr_t *, bcf1_t *, const char *, float **, int *) { REF_SHIM_TRAP("bcf_get_format_float"); }

}  // extern "C"
