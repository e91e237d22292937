/*
 * mfa_prefill.h -- C ABI of prefill attention over a KV cache: a BLOCK of new query rows per sequence, longer than a decode step
 * (chunked prefill, prefix reuse, a long speculative block), against keys and values that already live in the cache -- 16-bit or
 * FP8 (e4m3), contiguous or paged.  An extension of mfa_decode.h / mfa_kvcache.h, whose rules hold here word for word: plain
 * pointers and sizes, caller-owned device memory, status codes, validation before any GPU call, every refusal is
 * MFA_ERR_INVALID_ARGUMENT / MFA_ERR_UNSUPPORTED naming the requirement (there is no slow fallback), asynchronous launches on the
 * caller's HIP stream that copy nothing to the host and never synchronise (graph-capturable).
 *
 *   Q  [batches][heads][rows][D]            rows = capacity; sequence b uses its first queryLengths[b] rows
 *   K, V caches of heads / headsPerKeyValue heads: exactly decode's layouts -- contiguous with strides (token-major, zero batch
 *                                           stride, K / V slices of one allocation), or paged (pageSize a power of two 16 .. 1024,
 *                                           blockTable shared by K and V); see mfa_decode.h
 *   O  [batches][heads][rows][D]            the inputs' 16-bit type, or FP32
 *   L  [batches][heads][rows]               FP32, base-2 units: m + log2 l; NULL = not stored
 *
 * cacheLengths[b] (device, uint32, required): valid keys of sequence b INCLUDING the new tokens, which the caller has already
 * appended; clamped to `column`.  queryLengths[b] (device, uint32; NULL = every sequence has `rows`): the new rows of sequence b,
 * clamped to `rows`.  The host reads neither.  Rows at or past queryLengths[b] are neither read (Q) nor written (O, L).
 * Mask: with n = min(cacheLengths[b], column) and qn = queryLengths[b], row r < qn sees key c iff c < n and, with `causal`,
 * c <= r + max(n - qn, 0): decode's rule with the sequence's own row count.  A row without a visible key gets O = 0 and
 * L = -FLT_MAX.  Keys at or past n, the rest of a last page, pages the table does not name and table entries past the last page
 * are never loaded: they may hold anything, NaN or 0x7f included.  Scale 1 / sqrt(D).
 *
 * Quantisation.  The block is EMBEDDED in the params (cachePrecision, keyScale, valueScale) instead of a second mfa_kv_quant
 * argument as the FP8 decode entries take: the 16-bit and the e4m3 launch are one kernel family behind one template parameter (the
 * bytes are converted on their way into the workgroup's shared images; from there on the code is the same), there is no plan or
 * workspace the two would share through a common struct, and one set of five entries serves both.  Semantics are those of
 * mfa_kvcache.h: MFA_KV_E4M3 only (MFA_KV_E5M2 is MFA_ERR_UNSUPPORTED), per-K/V-head FP32 scales on the device, NULL = 1.0, the key
 * scale folded into the softmax scale and the value scale into the final normalisation.  Scales with a 16-bit cache are refused.
 *
 * What the kernels need: 16-bit Q (FP32: MFA_ERR_UNSUPPORTED); head dimensions 64, 128 and 256; Q, K, V, O 16-byte aligned; Q strides
 * multiples of 8 elements, O strides of 4; K / V strides multiples of 8 elements for a 16-bit cache and of 16 elements (= bytes) for
 * an e4m3 cache; heads a multiple of headsPerKeyValue G, G <= 32.  No upper limit on rows (G x rows <= 32 included: the same math
 * as decode).  The launch of these entries takes no workspace: it is not cut along the keys.  The entries of mfa_split.h are: a launch of
 * few row blocks over a long cache, cut into pieces of every row block's tiles with a workspace and a combine kernel.
 *
 * How a launch runs: one workgroup owns 128 packed rows of ONE K / V head of one sequence -- RB = 128 / G consecutive query rows
 * for each of the G query heads of the group -- so K and V are read once per group, not G times.  Grid = batches x K/V heads x
 * ceil(rows / RB); a block whose first row is at or past queryLengths[b] returns at once.
 */
#ifndef MFA_PREFILL_H
#define MFA_PREFILL_H

#include "mfa_kvcache.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_PREFILL_KEY_TILE 64        /* keys per tile */
#define MFA_PREFILL_PACKED_ROWS 128    /* packed rows of a workgroup: RB = 128 / G query rows of each of the G heads */
#define MFA_PREFILL_MAX_GROUP 32       /* G */

typedef struct mfa_prefill_params {
  uint32_t rows;                 /* capacity of Q, O, L along the rows */
  uint32_t column;               /* largest cache length of the launch */
  uint32_t heads, batches;       /* Hq, B */
  uint32_t headsPerKeyValue;     /* G; 0 = 1 */
  uint32_t causal;
  uint16_t headDimension;
  uint8_t precision;             /* MFA_FP16 / MFA_BF16: Q (and a 16-bit cache) */
  uint8_t outputPrecision;       /* `precision`, or MFA_FP32 */
  uint32_t pageSize;             /* 0 = contiguous */
  const uint32_t *cacheLengths;  /* device, [batches] */
  const uint32_t *queryLengths;  /* device, [batches]; NULL = rows */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged launches only */
  int64_t blockTableStride;      /* entries */
  int64_t leadingDimension[4], headStride[4], batchStride[4];   /* Q, K, V, O; elements.  K / V batchStride: contiguous only */
  int64_t pageStride[2];         /* K, V; elements */
  int64_t lHeadStride, lBatchStride;                            /* elements of L */
  uint32_t cachePrecision;       /* `precision`, or MFA_KV_E4M3 */
  uint32_t reserved;
  const float *keyScale, *valueScale;   /* device, [heads / headsPerKeyValue]; NULL = 1.0; e4m3 caches only */
} mfa_prefill_params;

/* zeroes the block; precision = outputPrecision = cachePrecision = MFA_BF16, headsPerKeyValue = 1, causal = 1 */
void mfa_prefill_params_init(mfa_prefill_params *params);

/* sizeof(mfa_prefill_params), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_prefill_params_size(void);
mfa_status mfa_prefill_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

mfa_status mfa_attention_prefill_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                        const mfa_prefill_params *params, void *stream);

/* what a launch with these parameters runs, as text: the kernel's name and the grid; nothing is launched */
mfa_status mfa_attention_prefill_launch_form(const mfa_prefill_params *params, char *out, size_t capacity);

/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_attention_prefill_time(const void *q, const void *k, const void *v, void *o, float *l,
                                      const mfa_prefill_params *params, void *stream, int warmup, int iterations,
                                      float *milliseconds);

/* the kernels' own tile-range function, on the host.  For the block of rows [firstRow, firstRow + blockRows) of a sequence of
 * `length` keys and `queryLength` rows: *end = the first 64-key tile no row of the block can see (tiles at or past it are never
 * loaded), *firstMasked = the first tile in which some row's causal frontier or `length` cuts (tiles below it run without the
 * per-element mask).  A block without a live row, or length 0: both 0. */
mfa_status mfa_attention_prefill_tile_range(uint32_t length, uint32_t queryLength, uint32_t firstRow, uint32_t blockRows,
                                            uint32_t causal, uint32_t *firstMasked, uint32_t *end);

#ifdef __cplusplus
}
#endif
#endif /* MFA_PREFILL_H */
