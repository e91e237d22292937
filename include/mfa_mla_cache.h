/*
 * mfa_mla_cache.h -- C ABI of what makes the latent cache of multi-head latent attention (mfa_mla.h) usable end to end: the launch
 * that APPENDS new rows to it (quantising them when the cache is FP8) and the decode launch that READS an FP8 latent cache.  To
 * mfa_mla.h what mfa_kvcache.h is to mfa_decode.h, whose rules hold here word for word: plain pointers and sizes, caller-owned device
 * memory, status codes, validation before any GPU call, every refusal names the requirement, asynchronous launches that copy nothing
 * to the host and never synchronise (graph-capturable).  No existing struct or entry changes.
 *
 * Format of an e4m3 latent cache.  One row of 576 BYTES per key: 512 latent bytes, then 64 rotary bytes, OCP FP8 E4M3 (`e4m3fn`, the
 * encoding of mfa_kvcache.h).  kvScale: a device FP32 array of ONE entry; NULL = 1.0.  A stored byte b stands for
 * kvScale[0] x e4m3(b) -- one scale for the whole row, latent and rotary part alike: the same bytes are key and value, so a second
 * scale would cost a second score accumulator.  The host never reads the scale; it folds into the softmax scale and into the final
 * normalisation, so the decode loop pays nothing for it.  Quantisation is mfa_kv_quantize_e4m3 (mfa_kvcache.h), unchanged -- the
 * contract between writer and reader; the append kernel produces exactly its bytes (it runs the same body).  Strides of an e4m3
 * cache are in elements = bytes and are multiples of 16; strides of a 16-bit cache are multiples of 8 elements, as in mfa_mla.h.
 *
 * Append.  latentNew [batches][rows][512] and ropeNew [batches][rows][64], both 16-bit (`precision`), each with its own leading
 * dimension and batch stride (multiples of 8 elements) and 16-byte aligned: frameworks hold the normalised latent and the rotated key
 * part as two tensors; a caller with a fused row of 576 passes p and p + 512 with one stride.  Row r of sequence b goes to key index
 * cacheLengths[b] - rows + r: cacheLengths ALREADY INCLUDES the new tokens, so one lengths array serves the append and the decode
 * that follows it.  A row whose index is negative, >= `column` (contiguous) or whose page index is >= blockTableStride (paged) is not
 * written; no other byte of the cache is touched.  Cache layouts are mfa_mla.h's: contiguous with batchStride (and `column`, the
 * capacity in keys), or paged (pageSize a power of two 16 .. 1024, a block table, pageStride).  cachePrecision is the rows' 16-bit
 * type (bits are copied; a non-NULL kvScale is refused) or MFA_KV_E4M3 (every element is mfa_kv_quantize_e4m3(x, kvScale[0]));
 * MFA_KV_E5M2 is MFA_ERR_UNSUPPORTED.  `rows` has no limit: a prompt's rows are appended in one launch.
 * Kernels: kv_latent_append_copy16 (a 16-bit cache), kv_latent_append_<bf16|f16>_e4m3.
 *
 * Decode over an e4m3 latent cache.  mfa_mla_decode_params unchanged (precision = the 16-bit type of Q; the KV strides in elements =
 * bytes, multiples of 16) plus mfa_mla_quant.  Q, O, L, the mask, lengths, empty sequences, never-loaded keys, packing into groups of
 * 32, the piece plan, mfa_attention_decode_piece_range and the workspace formula are those of mfa_mla.h; the workspace size equals
 * mfa_attention_mla_decode_workspace_size's, and the pieces are merged by the 16-bit launch's combine kernel.  A key that is never
 * loaded may hold anything, the NaN bytes 0x7f / 0xff included.
 * Kernels: attn_mla8_d576_<bf16|f16> (unsplit), attn_mla8_d576_<type>_k (a piece of the keys), attn_mla16_d576_<type>_combine.
 *
 * Deliberately not here: more than 32 packed rows per workgroup; a ragged append (per-sequence row counts) for the latent cache;
 * per-token or per-128-column scales, the 656-byte layout with a 16-bit rotary part included; e5m2; an FP8 Q or the FP8 matrix
 * instructions (the launch is bound by bytes, not by the matrix pipe); a window, sinks, a soft cap or trees on MLA; prefill over the
 * latent cache; compaction of a latent cache.
 */
#ifndef MFA_MLA_CACHE_H
#define MFA_MLA_CACHE_H

#include "mfa_kvcache.h"
#include "mfa_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_MLA_LATENT_DIMENSION 512  /* the latent part of a cache row (MFA_MLA_VALUE_DIMENSION) */
#define MFA_MLA_ROPE_DIMENSION 64     /* the rotary part behind it */

typedef struct mfa_mla_append_params {
  uint32_t rows;                 /* R new rows per sequence; no limit */
  uint32_t batches;
  uint32_t column;               /* capacity (keys) of a contiguous cache */
  uint32_t pageSize;             /* 0 = contiguous */
  uint16_t latentDimension;      /* 512 */
  uint16_t ropeDimension;        /* 64 */
  uint8_t precision;             /* MFA_FP16 / MFA_BF16: the new rows */
  uint8_t cachePrecision;        /* `precision`, or MFA_KV_E4M3 */
  uint16_t reserved;             /* 0 */
  const uint32_t *cacheLengths;  /* device, [batches]; includes the new rows */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged only */
  int64_t blockTableStride;
  int64_t leadingDimension[3], batchStride[3];   /* latentNew, ropeNew, kvCache; elements.  Cache batchStride: contiguous only */
  int64_t pageStride;            /* kvCache; elements */
  const float *kvScale;          /* device, one entry; NULL = 1.0; E4M3 caches only */
} mfa_mla_append_params;

/* zeroes the block; precision = cachePrecision = MFA_BF16, latentDimension = 512, ropeDimension = 64 */
void mfa_mla_append_params_init(mfa_mla_append_params *params);

/* sizeof(mfa_mla_append_params), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_mla_append_params_size(void);
mfa_status mfa_mla_append_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

mfa_status mfa_mla_cache_append_launch(const void *latentNew, const void *ropeNew, void *kvCache, const mfa_mla_append_params *params,
                                       void *stream);

typedef struct mfa_mla_quant {
  uint32_t cachePrecision;       /* MFA_KV_E4M3 */
  uint32_t reserved;
  const float *kvScale;          /* device, one entry; NULL = 1.0 */
} mfa_mla_quant;

/* zeroes the block; cachePrecision = MFA_KV_E4M3 */
void mfa_mla_quant_init(mfa_mla_quant *quant);

/* the four entries of mfa_mla.h for an E4M3 latent cache; bytes and pieces equal mfa_attention_mla_decode_workspace_size's */
mfa_status mfa_attention_mla_decode_fp8_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, uint64_t *bytes,
                                                       uint32_t *pieces);
mfa_status mfa_attention_mla_decode_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                               const mfa_mla_quant *quant, void *stream);
mfa_status mfa_attention_mla_decode_fp8_launch_form(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, char *out,
                                                    size_t capacity);
mfa_status mfa_attention_mla_decode_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                             const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_CACHE_H */
