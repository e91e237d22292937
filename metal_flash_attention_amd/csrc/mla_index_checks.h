// mla_index_checks.h -- what the two indexers' hosts share (attn_mla_index.hip: rows <= 32, one row per workgroup; attn_mla_index_prefill.hip:
// any number of rows, keys resident): the checks of mfa_mla_index_params in the order and words of include/mfa_mla_index.h, the argument
// block filled from the params, and the buffers of a stage.  What differs stays with each unit: its rows limit, its grid plan and its
// workspace.  Internal, not part of the ABI.
#pragma once
#include <cstring>
#include <string>

#include "../../include/mfa_mla_index.h"
#include "attn_mla_index.h"
#include "cache_launch.h"
#include "mfa_internal.h"

namespace mfa {

enum MlaIndexStage { MLAI_LOGITS = 1, MLAI_SELECT = 2, MLAI_TOPK = 3 };

inline uint64_t mlai_padded_column(uint32_t column) { return ((uint64_t)column + 3) & ~3ull; }

// the block itself; `maxRows` 0: no limit
inline mfa_status check_index_block(const mfa_mla_index_params *p, uint32_t maxRows) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->reserved != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_index_params.reserved must be 0, not " + std::to_string(p->reserved));
  if (p->rows == 0 || p->column == 0 || p->batches == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "rows, column and batches must be non-zero");
  if (maxRows && p->rows > maxRows)
    return fail(MFA_ERR_UNSUPPORTED, "the MLA indexer takes at most 32 rows per sequence, not rows = " + std::to_string(p->rows) +
                                         ": the limit of the sparse decode it feeds (a longer block of query rows is a prefill)");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  return MFA_OK;
}

// what the logits kernels read
inline mfa_status check_index_logits(const mfa_mla_index_params *p, uint32_t *pageShift) {
  if (p->indexDimension != MFA_MLA_INDEX_DIMENSION)
    return fail(MFA_ERR_UNSUPPORTED, "the MLA indexer is compiled for indexDimension = 128, not " + std::to_string(p->indexDimension));
  if (p->precision != MFA_BF16 && p->precision != MFA_FP16)
    return fail(MFA_ERR_UNSUPPORTED, "the MLA indexer reads 16-bit index queries and caches (precision MFA_BF16 or MFA_FP16); e4m3 index "
                                     "caches and FP32 have no kernel");
  if (p->indexHeads == 0 || p->indexHeads > MFA_MLA_INDEX_MAX_HEADS)
    return fail(MFA_ERR_INVALID_ARGUMENT, "indexHeads must be 1 .. 64, not " + std::to_string(p->indexHeads));
  mfa_status st = check_paging(p->pageSize, p->blockTable, p->blockTableStride, p->column, pageShift);
  if (st != MFA_OK) return st;
  static const char *names[2] = {"QI", "KI"};
  for (int i = 0; i < 2; ++i) {
    st = check_operand_strides(names[i], p->indexDimension, p->leadingDimension[i], i == 1 ? 0 : p->headStride[i],
                               i == 1 && p->pageSize ? p->pageStride : p->batchStride[i], 8, "(16-byte rows for QI and KI)");
    if (st != MFA_OK) return st;
  }
  if (p->rows > 1 && p->weightRowStride < (int64_t)p->indexHeads)
    return fail(MFA_ERR_INVALID_ARGUMENT, "weightRowStride must be at least indexHeads = " + std::to_string(p->indexHeads) + " elements, not " +
                                              std::to_string(p->weightRowStride));
  return MFA_OK;
}

// what the select kernels read and write
inline mfa_status check_index_select(const mfa_mla_index_params *p) {
  if (p->topk == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "topk must be at least 1 (the slots of a row's list)");
  if (p->indexRowStride < (int64_t)p->topk)
    return fail(MFA_ERR_INVALID_ARGUMENT, "indexRowStride must be at least topk = " + std::to_string(p->topk) + " entries, not " +
                                              std::to_string(p->indexRowStride));
  if (p->column > 0x7FFFFFFFu) return fail(MFA_ERR_INVALID_ARGUMENT, "column must be below 2^31 keys for the selection (its position arithmetic is 32-bit)");
  if ((uint64_t)p->rows * p->batches > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "rows x batches must fit a grid of 2^31 - 1 workgroups");
  return MFA_OK;
}

// the logits of a launch that is not the chain: the caller's, by its strides
inline mfa_status check_index_logit_stride(const mfa_mla_index_params *p) {
  if (p->logitRowStride < (int64_t)p->column)
    return fail(MFA_ERR_INVALID_ARGUMENT, "logitRowStride must be at least column = " + std::to_string(p->column) + " elements, not " +
                                              std::to_string(p->logitRowStride));
  return MFA_OK;
}

// the fields every kernel of both units reads (the logits' strides, the plan and the buffers are the unit's)
inline void fill_index_args(MlaIndexArgs &a, const mfa_mla_index_params *p, uint32_t pageShift) {
  a.lengths = p->cacheLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride;
  a.wrs = p->weightRowStride; a.wbs = p->weightBatchStride;
  a.irs = p->indexRowStride; a.ibs = p->indexBatchStride;
  a.R = p->rows; a.H = p->indexHeads; a.batches = p->batches; a.column = p->column; a.topk = p->topk;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0;
}

// the buffers of a launch into the argument block: what the stage does not take is null and not looked at
inline mfa_status bind_index(MlaIndexArgs &a, int stage, const void *qi, const float *w, const void *ki, float *logits, int32_t *indices) {
  mfa_status st = MFA_OK;
  if (stage & MLAI_LOGITS) {
    st = check_buffers({qi, ki}, "QI and KI");
    if (st == MFA_OK && !w) st = fail(MFA_ERR_INVALID_ARGUMENT, "W is required (device FP32 [batches][rows][indexHeads])");
    if (st == MFA_OK) st = check_float_arrays({w}, "W");
    if (st != MFA_OK) return st;
    a.q = (const char *)qi; a.w = w; a.k = (const char *)ki;
  }
  if (stage != MLAI_TOPK) {
    if (!logits) return fail(MFA_ERR_INVALID_ARGUMENT, "logits is required (device FP32 [batches][rows][logitRowStride])");
    if ((st = check_float_arrays({logits}, "logits")) != MFA_OK) return st;
    a.logits = logits;
  }
  if (stage & MLAI_SELECT) {
    if (!indices) return fail(MFA_ERR_INVALID_ARGUMENT, "indices is required (device int32 [batches][rows][topk])");
    if ((uintptr_t)indices % 4 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "indices must be 4-byte aligned");
    a.indices = indices;
  }
  return MFA_OK;
}

} // namespace mfa
