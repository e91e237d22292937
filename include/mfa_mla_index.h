/*
 * mfa_mla_index.h -- C ABI of the MLA SPARSE INDEXER: the producer of the per-row key lists that mfa_mla_sparse.h consumes -- the
 * "lightning indexer" of DeepSeek-V3.2, which scores every key of a sequence with a few small index heads and keeps the topk best per
 * query token.  Two launches and their chain: the INDEX LOGITS of every visible key, on matrix instructions, and a deterministic
 * TOP-K SELECTION that writes lists exactly as the sparse decode reads them.  An extension of this port (the reference has no such
 * entry) beside mfa_mla.h, whose rules hold here: plain pointers and sizes, caller-owned device memory, status codes, nothing aborts,
 * every refusal before any GPU call and naming the requirement, asynchronous launches on the caller's HIP stream.  A launch copies
 * nothing to the host and never synchronises, so it can sit in a captured graph.  No existing struct or entry changes.
 *
 *   QI      [batches][indexHeads][rows][Di]   the index queries, MFA_BF16 or MFA_FP16; Di = indexDimension = 128
 *   W       [batches][rows][indexHeads]       FP32 per-row, per-head weights, heads contiguous.  The MODEL's own: the caller has folded
 *                                             in any softmax or quantisation scale.  They may be negative.
 *   KI      index key cache: one "head"; key c of sequence b is a row of Di 16-bit values, in mfa_mla.h's cache layouts with Di in
 *           place of Dk (below)
 *   logits  [batches][rows][logitRowStride]   FP32: the logits launch's output and the select launch's input
 *   indices [batches][rows][topk]             int32 key POSITIONS: indexRowStride >= topk and indexBatchStride are the very fields of
 *                                             mfa_mla_sparse, so the result is handed on unchanged
 *
 * Only Di = 128 is served; any other is MFA_ERR_UNSUPPORTED naming the number.  indexHeads is 1 .. MFA_MLA_INDEX_MAX_HEADS = 64, any
 * value; heads at or past indexHeads are never loaded and contribute nothing.  rows <= 32, the limit of the sparse decode this feeds.
 *
 * Visibility is mfa_mla.h's rule.  cacheLengths[b] (device, uint32, required; the host never reads it) counts the valid keys of
 * sequence b INCLUDING the R new tokens.  With n = min(cacheLengths[b], column), row r sees the PREFIX [0, v): v = n without `causal`,
 * v = min(n, r + max(n - rows, 0) + 1) with it.
 *
 * Layouts (strides in elements; operand 0 is QI, operand 1 is KI):
 *   contiguous (pageSize = 0): key c of sequence b at  KI + b batchStride + c leadingDimension  (batchStride 0 shares one cache; any
 *                              row stride that is a multiple of 8 elements)
 *   paged (pageSize a power of two, 16 .. 1024): blockTable (device, int32, [batches][blockTableStride]) entry (b, i) is the page of
 *                              keys i pageSize .. (i + 1) pageSize - 1; key c lives at KI + page pageStride + (c % pageSize)
 *                              leadingDimension.  Entries past a sequence's last page are never read.
 * What the kernels need (anything else is MFA_ERR_INVALID_ARGUMENT naming the requirement; there is no slow fallback): QI and KI
 * 16-byte aligned with strides that are multiples of 8 elements; W, logits and indices 4-byte aligned; logitRowStride >= column;
 * indexRowStride >= topk; the workspace of the chained entry 16-byte aligned.
 *
 * mfa_mla_index_logits_launch.  For every row and every visible position c < v:
 *     logits[b][r][c] = sum over h of  W[b][r][h] x max(q_I[b][h][r] . k_I[b][c], 0)       accumulated in FP32 starting from +0
 * Positions at or past v are NOT WRITTEN.  Keys at or past n, the rest of a last page, pages the table does not name and table entries
 * past the last page are NEVER LOADED: they may hold anything, NaN included.  Work split: a workgroup is four waves that serve ONE
 * (sequence, row) and a tile of MFA_MLA_INDEX_KEY_STEP x 4 x steps keys; a wave keeps the row's queries and weights in registers and
 * scores 32 keys per step, heads on the M side of v_mfma_f32_32x32x16, keys on the N side.  Grid: tiles x rows x batches, the rows of
 * a sequence neighbours.  A tile wholly at or past v returns at once; outputs are independent per key, there is no combine pass.
 *
 * mfa_mla_index_select_launch.  For every row it reads only logits[b][r][0 .. v) and writes the row's list.  Membership: the
 * min(topk, v) positions that come first under the order "larger logit first, ties broken by lower position first".  Logits are
 * compared as the total order of their FP32 bit patterns, key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): -0 < +0, and a NaN
 * sorts where its bits put it (callers pass none).  Layout of the list: the selected positions in ASCENDING POSITION ORDER, then -1 in
 * every remaining slot up to topk; nothing past slot topk - 1 is written.  If v <= topk the list is 0, 1, ..., v - 1, -1, ...; a row
 * with v = 0 is all -1.  The result is a pure function of the inputs: a most-significant-digit-first radix select narrows to the
 * threshold key, and one ordered pass with a workgroup prefix scan writes the positions, so nothing depends on scheduling.  One
 * workgroup per (sequence, row).  topk >= 1 is otherwise free.
 *
 * mfa_mla_index_topk_launch.  The two launches back to back on the stream, with the logits in the caller's `workspace`, laid out
 * [batches][rows][column rounded up to 4] (logitRowStride and logitBatchStride are not looked at).  mfa_mla_index_workspace_size says
 * how many bytes; a NULL or short workspace is refused by name.  Its result is the select launch applied to the logits launch, bit
 * for bit.
 *
 * Kernels: attn_mlai_d128_<bf16|f16> (logits), attn_mlai_select.
 *
 * Deliberately not here: e4m3 index caches and per-key scales; an FP8 matrix-instruction path; writing the index cache (the caller
 * stores its index keys with plain torch); rows > 32 under THESE entries (a prompt chunk is mfa_mla_index_prefill.h); cutting one
 * row's selection across several workgroups; physical-slot indices.
 */
#ifndef MFA_MLA_INDEX_H
#define MFA_MLA_INDEX_H

#include "mfa_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_MLA_INDEX_DIMENSION 128   /* Di */
#define MFA_MLA_INDEX_MAX_HEADS 64
#define MFA_MLA_INDEX_KEY_STEP 32     /* keys a wave scores per step; a workgroup's four waves take 128 */

typedef struct mfa_mla_index_params {
  uint32_t rows;                 /* R <= 32 */
  uint32_t column;               /* largest cache length of the launch */
  uint32_t indexHeads, batches;  /* Hi in 1 .. 64, B */
  uint32_t causal;
  uint16_t indexDimension;       /* Di = 128 */
  uint8_t precision;             /* MFA_FP16 / MFA_BF16: QI and the index cache */
  uint8_t reserved;              /* 0 */
  uint32_t pageSize;             /* 0 = contiguous */
  uint32_t topk;                 /* slots of a row's list, >= 1 (the logits launch does not look at it) */
  const uint32_t *cacheLengths;  /* device, [batches] */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged launches only */
  int64_t blockTableStride;      /* entries */
  int64_t leadingDimension[2], headStride[2], batchStride[2];   /* QI, KI; elements.  KI: headStride unused, batchStride contiguous only */
  int64_t pageStride;            /* KI; elements */
  int64_t weightRowStride, weightBatchStride;   /* elements of W */
  int64_t logitRowStride, logitBatchStride;     /* elements of logits; logitRowStride >= column */
  int64_t indexRowStride, indexBatchStride;     /* entries of indices; indexRowStride >= topk */
  void *workspace;               /* the chained entry's logits */
  uint64_t workspaceBytes;
} mfa_mla_index_params;

/* zeroes the block; precision = MFA_BF16, indexDimension = 128, causal = 1 */
void mfa_mla_index_params_init(mfa_mla_index_params *params);

/* sizeof(mfa_mla_index_params), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_mla_index_params_size(void);
mfa_status mfa_mla_index_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* *bytes: what mfa_mla_index_topk_launch needs, batches x rows x (column rounded up to 4) x 4.  The workspace the params may already
 * carry is not looked at. */
mfa_status mfa_mla_index_workspace_size(const mfa_mla_index_params *params, uint64_t *bytes);

mfa_status mfa_mla_index_logits_launch(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                       void *stream);
/* what a launch with these parameters runs, as text: the kernel's name, the grid with its factors, the layout */
mfa_status mfa_mla_index_logits_launch_form(const mfa_mla_index_params *params, char *out, size_t capacity);
/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_mla_index_logits_time(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                     void *stream, int warmup, int iterations, float *milliseconds);

mfa_status mfa_mla_index_select_launch(const float *logits, int32_t *indices, const mfa_mla_index_params *params, void *stream);
mfa_status mfa_mla_index_select_launch_form(const mfa_mla_index_params *params, char *out, size_t capacity);
mfa_status mfa_mla_index_select_time(const float *logits, int32_t *indices, const mfa_mla_index_params *params, void *stream, int warmup,
                                     int iterations, float *milliseconds);

mfa_status mfa_mla_index_topk_launch(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                     void *stream);
mfa_status mfa_mla_index_topk_launch_form(const mfa_mla_index_params *params, char *out, size_t capacity);
mfa_status mfa_mla_index_topk_time(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                   void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_INDEX_H */
