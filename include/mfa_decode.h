/*
 * mfa_decode.h -- C ABI of decode attention: R new query rows per sequence (R = 1, or a few speculative tokens)
 * against a long cache of keys and values, the shape of token-by-token generation.  An extension of this port (the
 * reference has no such entry); same rules as mfa.h: plain pointers and sizes, caller-owned device memory, status
 * codes, nothing aborts, validation before any GPU call, asynchronous launches on the caller's HIP stream.  A launch
 * copies nothing to the host and never synchronises, so it can sit in a captured graph.
 *
 *   Q  [batches][heads][rows][D]            rows = R, the same for every batch entry
 *   K, V caches of heads / headsPerKeyValue heads; query head h reads K / V head h / G (mfa_launch_params.headsPerKeyValue)
 *   O  [batches][heads][rows][D]            the inputs' 16-bit type, or FP32
 *   L  [batches][heads][rows]               FP32, base-2 units: m + log2 l, the forward kernel's storage; NULL = not stored.
 *                                           With L a caller merges results across cache shards.
 *
 * cacheLengths[b] (device, uint32, required): valid keys of sequence b INCLUDING the R new tokens, which the caller has
 * already written into the cache; clamped to `column`.  The host never reads it.  The cache is never written.
 * Mask: with `causal`, row r of sequence b sees key c iff c <= r + max(cacheLengths[b] - R, 0) and c < cacheLengths[b]
 * (the per-batch-length rule of mfa.h); without it every row sees every valid key.  A sequence of length 0 gets O = 0 and
 * L = -FLT_MAX.  Keys at or past a length, the rest of a last page and pages the table does not name are never loaded:
 * they may hold anything, NaN included.  Scale 1 / sqrt(D).
 *
 * Layouts (strides in elements, per operand Q, K, V, O):
 *   contiguous (pageSize = 0): key c of K / V head j of sequence b at  K + j headStride + b batchStride + c leadingDimension
 *                              (a token-major [B][C][Hkv][D] cache is just strides; batchStride 0 shares one cache)
 *   paged (pageSize a power of two, 16 .. 1024): blockTable (device, int32, [batches][blockTableStride]) entry (b, i) is the
 *                              page of keys i pageSize .. (i + 1) pageSize - 1; key c of head j lives at
 *                              K + page pageStride + j headStride + (c % pageSize) leadingDimension.  Entries past a
 *                              sequence's last page are never read.  K and V have their own strides and share the table.
 *
 * What the kernels need (anything else is MFA_ERR_INVALID_ARGUMENT naming the requirement; there is no slow fallback):
 *   Q, K, V 16-byte aligned with strides that are multiples of 8 elements; O 16-byte aligned with strides that are multiples
 *   of 4 elements; the workspace 16-byte aligned.  16-bit inputs only (FP32 caches: MFA_ERR_UNSUPPORTED); head dimensions 64,
 *   128 and 256 (anything else: MFA_ERR_UNSUPPORTED); packed rows M = G x R <= 32 (a longer block of rows is a prefill:
 *   mfa_attention_kernel_launch).
 *
 * How a launch runs: one workgroup packs the G query heads x R rows of one K / V head as the rows of one matrix tile, so K and
 * V are read once per launch, not G times.  With a workspace the keys are cut into `pieces` (chosen on the host from
 * batches x K/V heads and `column` only); every piece of sequence b takes an equal share, in whole 64-key tiles, of that
 * sequence's OWN length (mfa_attention_decode_piece_range is the function the kernel runs), writes un-normalised O, m, l in
 * FP32 to the workspace and a second kernel merges them.  Without a workspace (or when the plan has one piece) one kernel
 * does it all.
 */
#ifndef MFA_DECODE_H
#define MFA_DECODE_H

#include "mfa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_DECODE_KEY_TILE 64           /* keys per tile: pieces are whole tiles, except a sequence's last */
#define MFA_DECODE_MAX_PACKED_ROWS 32    /* G x R */
#define MFA_DECODE_WORKGROUP_TARGET 512  /* workgroups a split aims at: two per compute unit of a 256-CU chip */
#define MFA_DECODE_MAX_PIECES 64

typedef struct mfa_decode_params {
  uint32_t rows;                 /* R */
  uint32_t column;               /* largest cache length of the launch */
  uint32_t heads, batches;       /* Hq, B */
  uint32_t headsPerKeyValue;     /* G; 0 = 1 */
  uint32_t causal;
  uint16_t headDimension;
  uint8_t precision;             /* MFA_FP16 / MFA_BF16: Q, K and V */
  uint8_t outputPrecision;       /* `precision`, or MFA_FP32 */
  uint32_t pageSize;             /* 0 = contiguous */
  const uint32_t *cacheLengths;  /* device, [batches] */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged launches only */
  int64_t blockTableStride;      /* entries */
  int64_t leadingDimension[4], headStride[4], batchStride[4];   /* Q, K, V, O; elements.  K / V batchStride: contiguous only */
  int64_t pageStride[2];         /* K, V; elements */
  int64_t lHeadStride, lBatchStride;                            /* elements of L */
  void *workspace;
  uint64_t workspaceBytes;
} mfa_decode_params;

/* zeroes the block; precision = outputPrecision = MFA_BF16, headsPerKeyValue = 1, causal = 1 */
void mfa_decode_params_init(mfa_decode_params *params);

/* bytes a launch wants to be cut along the keys: pieces x batches x heads x rows x (D + 2) x 4 (the forward split's formula),
 * 0 when the plan has one piece.  A launch without a workspace runs unsplit and is still correct; one whose workspace is smaller
 * than this is MFA_ERR_INVALID_ARGUMENT naming the byte count. */
mfa_status mfa_attention_decode_workspace_size(const mfa_decode_params *params, uint64_t *bytes);

mfa_status mfa_attention_decode_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                       const mfa_decode_params *params, void *stream);

/* what a launch with these parameters runs, as text: the kernels' names, the grid, the piece count */
mfa_status mfa_attention_decode_launch_form(const mfa_decode_params *params, char *out, size_t capacity);

/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_attention_decode_time(const void *q, const void *k, const void *v, void *o, float *l,
                                     const mfa_decode_params *params, void *stream, int warmup, int iterations,
                                     float *milliseconds);

/* the kernels' own piece -> key-range function, on the host: keys [*begin, *end) of piece `piece` of `pieces` for a sequence
 * of `length` keys */
mfa_status mfa_attention_decode_piece_range(uint32_t length, uint32_t pieces, uint32_t piece, uint32_t *begin, uint32_t *end);

#ifdef __cplusplus
}
#endif
#endif /* MFA_DECODE_H */
