/*
 * mfa_mla_prefill.h -- C ABI of multi-head latent attention (MLA) PREFILL in its "absorbed" form over the compressed KV cache of
 * mfa_mla.h: a BLOCK of new query rows per sequence, of any length (chunked prefill, prefix reuse, the extend step after a cache hit,
 * a long draft block), against the 576-wide rows the append kernel of mfa_mla_cache.h wrote.  An extension of this port beside
 * mfa_mla.h, whose rules hold here word for word: plain pointers and sizes, caller-owned device memory, status codes, nothing aborts,
 * validation before any GPU call, every refusal is MFA_ERR_INVALID_ARGUMENT / MFA_ERR_UNSUPPORTED naming the requirement (there is no
 * slow fallback), asynchronous launches on the caller's HIP stream that copy nothing to the host and never synchronise
 * (graph-capturable).  It is in no family table and takes no option; no existing struct or entry changes.
 *
 *   Q  [batches][heads][rows][Dk]           rows = capacity; sequence b uses its first queryLengths[b] rows; Dk = headDimension = 576
 *   KV cache: exactly mfa_mla.h's layouts -- one "head"; key c of sequence b is a row of Dk 16-bit values, whose first Dv =
 *                                           valueDimension = 512 are also the value row
 *   O  [batches][heads][rows][Dv]           the inputs' 16-bit type, or FP32
 *   L  [batches][heads][rows]               FP32, base-2 units: m + log2 l; NULL = not stored
 *
 * Strides are per operand (row, head, batch), in elements, as in mfa_mla_decode_params: a token-major Q / O ([batches][rows][heads][..]
 * seen through strides) is a plain launch.  Only (Dk, Dv) = (576, 512) in MFA_BF16 or MFA_FP16 is served; any other pair is
 * MFA_ERR_UNSUPPORTED naming both numbers.  rows >= 1, no upper limit; rows <= 32 is served too (the same math as mfa_mla.h's unsplit
 * launch, bit for bit).
 *
 * scale (float): the softmax scale in natural units, applied to q . k -- the MODEL's own, not 1 / sqrt(Dk).  Required: finite and > 0,
 * there is no default; a zero or non-finite value is MFA_ERR_INVALID_ARGUMENT naming the field.  The kernel uses fl(scale x log2 e).
 *
 * cacheLengths[b] (device, uint32, required): valid keys of sequence b INCLUDING the new tokens, which the caller has already
 * appended; clamped to `column`.  queryLengths[b] (device, uint32; NULL = every sequence has `rows`): the new rows of sequence b,
 * clamped to `rows`.  The host reads neither.  Rows at or past queryLengths[b] are neither read (Q) nor written (O, L).
 * Mask: with n = min(cacheLengths[b], column) and qn = queryLengths[b], row r < qn sees key c iff c < n and, with `causal`,
 * c <= r + max(n - qn, 0): decode's rule with the sequence's own row count.  A row without a visible key gets O = 0 and
 * L = -FLT_MAX.  Keys at or past n, the rest of a last page, pages the table does not name and table entries past the last page
 * are never loaded: they may hold anything, NaN included.  The cache is never written.
 *
 * Layouts of the cache (mfa_mla.h): contiguous (pageSize = 0; any row stride that is a multiple of 8 elements, batchStride 0 shares
 * one cache) or paged (pageSize a power of two, 16 .. 1024, with blockTable, blockTableStride and pageStride).
 * What the kernels need (anything else is MFA_ERR_INVALID_ARGUMENT naming the requirement): Q and KV 16-byte aligned with strides that
 * are multiples of 8 elements; O 16-byte aligned with strides that are multiples of 4 elements.  heads >= 1 is otherwise free.
 *
 * Packing.  The M = rows x heads rows of a sequence are packed ROW-major: packed p = row x heads + head, so that the rows of a
 * workgroup share a causal frontier as nearly as they can.  They are cut into blocks of MFA_MLA_PREFILL_PACKED_ROWS = 64 packed rows;
 * one workgroup serves one block of one sequence: grid = batches x ceil(rows x heads / 64).  A block whose first row is at or past
 * queryLengths[b] returns at once.  A block seam may fall inside a row's heads; the last block may be partial.
 *
 * How a block runs: it walks the keys from 0 in steps of MFA_MLA_PREFILL_KEY_STEP = 32 up to the `end` of
 * mfa_attention_mla_prefill_step_range; every cache row of a step is fetched ONCE and serves all 64 packed rows and both products.
 * The steps below `firstMasked` run without the per-element mask.  For every packed row the arithmetic is that of mfa_mla.h's unsplit
 * kernel: the result of a row does not depend on the block it falls in, nor on how a prompt is cut into launches.
 *
 * Kernels: attn_mla16p_d576_<bf16|f16>.
 *
 * Deliberately not here: key pieces and a combine pass for launches of few blocks over a long cache (this launch takes no workspace);
 * e4m3 latent caches; ragged (packed-axis) rows; lists of key positions; a window, sinks, a soft cap or trees.
 */
#ifndef MFA_MLA_PREFILL_H
#define MFA_MLA_PREFILL_H

#include "mfa_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_MLA_PREFILL_PACKED_ROWS 64   /* packed rows (row x heads + head) of one workgroup */
#define MFA_MLA_PREFILL_KEY_STEP 32      /* keys per step */

typedef struct mfa_mla_prefill_params {
  uint32_t rows;                 /* capacity of Q, O, L along the rows; >= 1 */
  uint32_t column;               /* largest cache length of the launch */
  uint32_t heads, batches;       /* H, B */
  uint32_t causal;
  uint16_t headDimension;        /* Dk = 576 */
  uint16_t valueDimension;       /* Dv = 512 */
  uint8_t precision;             /* MFA_FP16 / MFA_BF16: Q and the cache */
  uint8_t outputPrecision;       /* `precision`, or MFA_FP32 */
  uint16_t reserved;             /* 0 */
  float scale;                   /* softmax scale, natural units; required: finite, > 0 */
  uint32_t pageSize;             /* 0 = contiguous */
  const uint32_t *cacheLengths;  /* device, [batches] */
  const uint32_t *queryLengths;  /* device, [batches]; NULL = rows */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged launches only */
  int64_t blockTableStride;      /* entries */
  int64_t leadingDimension[3], headStride[3], batchStride[3];   /* Q, KV, O; elements.  KV: headStride unused, batchStride contiguous only */
  int64_t pageStride;            /* KV; elements */
  int64_t lHeadStride, lBatchStride;                            /* elements of L */
} mfa_mla_prefill_params;

/* zeroes the block; precision = outputPrecision = MFA_BF16, headDimension = 576, valueDimension = 512, causal = 1.  scale stays 0:
 * the caller must set it */
void mfa_mla_prefill_params_init(mfa_mla_prefill_params *params);

/* sizeof(mfa_mla_prefill_params), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_mla_prefill_params_size(void);
mfa_status mfa_mla_prefill_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

mfa_status mfa_attention_mla_prefill_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                            void *stream);

/* what a launch with these parameters runs, as text: the kernel's name and the grid; nothing is launched */
mfa_status mfa_attention_mla_prefill_launch_form(const mfa_mla_prefill_params *params, char *out, size_t capacity);

/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_attention_mla_prefill_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                          void *stream, int warmup, int iterations, float *milliseconds);

/* the kernels' own range function, on the host.  For the block of the 64 packed rows from `firstPacked` (p = row x heads + head) of a
 * sequence of `length` keys and `queryLength` rows, in 32-key steps: *end = the first step no live row of the block can see (steps at
 * or past it are never loaded), *firstMasked = the first step in which some row's causal frontier or `length` cuts (steps below it run
 * without the per-element mask).  A block without a live row, or length 0: both 0. */
mfa_status mfa_attention_mla_prefill_step_range(uint32_t length, uint32_t queryLength, uint32_t firstPacked, uint32_t heads,
                                                uint32_t causal, uint32_t *firstMasked, uint32_t *end);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_PREFILL_H */
