/*
 * mfa_kvcache.h -- C ABI of the FP8 KV cache: the launch that APPENDS new key / value rows to a cache (quantising them when the
 * cache is FP8) and the decode launch that READS an FP8 cache.  An extension of mfa_decode.h, whose rules hold here word for word:
 * plain pointers and sizes, caller-owned device memory, status codes, validation before any GPU call, every refusal names the
 * requirement, asynchronous launches that copy nothing to the host and never synchronise (graph-capturable).
 *
 * Format.  A cache element is one byte, OCP FP8 E4M3 (`e4m3fn`: no infinities, +-448 largest, 0x7f / 0xff NaN) -- the encoding
 * gfx950 converts in hardware, not MI300's `fnuz`.  E5M2 caches are MFA_ERR_UNSUPPORTED.
 *
 * Scales.  keyScale / valueScale: device FP32 arrays of heads / headsPerKeyValue entries, one per K / V head; NULL = 1.0.  The
 * stored byte b of head j represents  value ~ scale[j] x e4m3(b).  The host never reads them.  Per head, not per token: the K
 * scale folds into the softmax scale and the V scale into the final normalisation, so the decode loop pays nothing for them.
 *
 * Quantisation is mfa_kv_quantize_e4m3 below -- the contract between writer and reader; the append kernel produces exactly its
 * bytes (it runs the same body).
 *
 * Append.  kNew, vNew [batches][heads][rows][D] (16-bit, strided like decode's Q); row r of sequence b goes to key index
 * cacheLengths[b] - rows + r: cacheLengths ALREADY INCLUDES the new tokens, so one lengths array serves the append and the decode
 * that follows it.  A row whose index is negative, >= `column` (contiguous) or whose page index is >= blockTableStride (paged) is
 * not written; no other byte of the cache is touched.  Cache layouts are decode's: contiguous with strides, or paged (pageSize a
 * power of two 16 .. 1024, K and V share the table).  The cache is the rows' 16-bit type (bits are copied) or E4M3.
 *   All four buffers 16-byte aligned; strides of the sources and of a 16-bit cache multiples of 8 elements, strides of an E4M3
 *   cache multiples of 16 elements; head dimensions 64, 128 and 256.
 *
 * Decode over an E4M3 cache.  mfa_decode_params unchanged (precision = the 16-bit type of Q; K / V strides in elements = bytes,
 * multiples of 16) plus mfa_kv_quant.  Q, O, L, the mask, length, poison and piece rules, the piece plan and the workspace formula
 * are those of mfa_decode.h; the pieces are merged by the 16-bit launch's combine kernel.
 */
#ifndef MFA_KVCACHE_H
#define MFA_KVCACHE_H

#include "mfa_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_KV_E4M3 16   /* cache precision codes beside mfa_precision's 16-bit types */
#define MFA_KV_E5M2 17   /* recognised only to be refused */

/* round-to-nearest-even e4m3 of clamp(x / scale, -448, +448); IEEE FP32 division; saturates, never NaN from a finite input;
 * -0 is kept; NaN -> NaN (0x7f with the sign bit) */
uint8_t mfa_kv_quantize_e4m3(float x, float scale);
float mfa_kv_dequantize_e4m3(uint8_t byte);

typedef struct mfa_kv_append_params {
  uint32_t rows;                 /* R new rows per sequence */
  uint32_t heads;                /* K / V heads */
  uint32_t batches;
  uint32_t column;               /* capacity (keys) of a contiguous cache */
  uint16_t headDimension;
  uint8_t precision;             /* MFA_FP16 / MFA_BF16: the new rows */
  uint8_t cachePrecision;        /* `precision`, or MFA_KV_E4M3 */
  uint32_t pageSize;             /* 0 = contiguous */
  const uint32_t *cacheLengths;  /* device, [batches]; includes the new rows */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged only */
  int64_t blockTableStride;
  int64_t leadingDimension[4], headStride[4], batchStride[4];   /* kNew, vNew, kCache, vCache; elements.  Cache batchStride: contiguous only */
  int64_t pageStride[2];         /* kCache, vCache; elements */
  const float *keyScale, *valueScale;   /* device, [heads]; NULL = 1.0; E4M3 caches only */
} mfa_kv_append_params;

/* zeroes the block; precision = cachePrecision = MFA_BF16 */
void mfa_kv_append_params_init(mfa_kv_append_params *params);

mfa_status mfa_kv_cache_append_launch(const void *kNew, const void *vNew, void *kCache, void *vCache,
                                      const mfa_kv_append_params *params, void *stream);

typedef struct mfa_kv_quant {
  uint32_t cachePrecision;       /* MFA_KV_E4M3 */
  uint32_t reserved;
  const float *keyScale, *valueScale;   /* device, [heads / headsPerKeyValue]; NULL = 1.0 */
} mfa_kv_quant;

/* zeroes the block; cachePrecision = MFA_KV_E4M3 */
void mfa_kv_quant_init(mfa_kv_quant *quant);

/* the four entries of mfa_decode.h for an E4M3 cache; the workspace size equals mfa_attention_decode_workspace_size */
mfa_status mfa_attention_decode_fp8_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint64_t *bytes);
mfa_status mfa_attention_decode_fp8_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                           const mfa_decode_params *params, const mfa_kv_quant *quant, void *stream);
mfa_status mfa_attention_decode_fp8_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, char *out, size_t capacity);
mfa_status mfa_attention_decode_fp8_time(const void *q, const void *k, const void *v, void *o, float *l,
                                         const mfa_decode_params *params, const mfa_kv_quant *quant, void *stream, int warmup,
                                         int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_KVCACHE_H */
