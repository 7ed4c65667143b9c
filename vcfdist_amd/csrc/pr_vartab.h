// pr_vartab.h -- what the entries that join the two callsets inside a supercluster share on the host (vpr_errclass,
// pr_errclass.hip; vpr_matchkind, pr_matchkind.hip): the check of the caller's variant tables against the resident batch and
// their upload as one device block that lives as long as the call.  `entry` is the caller's name, for the messages.
#pragma once

#include "pr_host.h"
#include "pr_varscan.h"

// The variant tables of one call on the device: the seven columns and the ALT pool of every hap slot in one block.  The block
// goes when the object does, after the handle's stream has drained (the kernels that read it are queued there).
struct VarTables {
    vpr_handle *h = nullptr;
    uint8_t *blk = nullptr;
    VsCols cols[VPR_HAPS];
    VarTables() = default;
    VarTables(const VarTables &) = delete;
    VarTables &operator=(const VarTables &) = delete;
    ~VarTables();
};

// The preconditions of include/vcfdist_errclass.h / vcfdist_matchkind.h on the variant tables: n_sc and the per-slot variant counts
// equal the resident batch's (VPR_ERR_STATE), var_off starts at 0 and is monotone, var_pos is non-decreasing inside a supercluster,
// allele offsets and lengths are non-negative (VPR_ERR_ARG).  pool_len: per slot the bytes of allele_pool the variants' ALT alleles
// name (the pool's extent is not part of vpr_variants).
int vartab_check(vpr_handle *h, const char *entry, const vpr_variants *v, size_t pool_len[VPR_HAPS]);
// The checked tables into one device block, copied on the handle's stream; T->cols name its pieces (ref_off stays null).
int vartab_upload(vpr_handle *h, const char *entry, const vpr_variants *v, const size_t pool_len[VPR_HAPS], VarTables *T);
