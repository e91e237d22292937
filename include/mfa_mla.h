/*
 * mfa_mla.h -- C ABI of multi-head latent attention (MLA) decode in its "absorbed" form over a COMPRESSED KV cache: the decode step of
 * DeepSeek-V2 / V3 / R1 and Kimi K2.  The cache holds ONE row of Dk = 576 values per token -- a 512-wide latent followed by a 64-wide
 * rotary part -- and every query head reads that same row, all Dk columns as its key and the first Dv = 512 columns as its value.  An
 * extension of this port (the reference has no such entry) beside mfa_decode.h, whose rules hold here: plain pointers and sizes,
 * caller-owned device memory, status codes, nothing aborts, validation before any GPU call, asynchronous launches on the caller's HIP
 * stream.  A launch copies nothing to the host and never synchronises, so it can sit in a captured graph.  No existing struct or entry
 * changes.
 *
 *   Q  [batches][heads][rows][Dk]           rows = R, the same for every batch entry; Dk = headDimension = 576
 *   KV cache: one "head"; key c of sequence b is a row of Dk 16-bit values, whose first Dv = valueDimension = 512 are also the value row
 *   O  [batches][heads][rows][Dv]           the inputs' 16-bit type, or FP32
 *   L  [batches][heads][rows]               FP32, base-2 units: m + log2 l, the forward kernel's storage; NULL = not stored.
 *
 * Only (Dk, Dv) = (576, 512) in MFA_BF16 or MFA_FP16 is served; any other pair is MFA_ERR_UNSUPPORTED naming both numbers.
 *
 * scale (float): the softmax scale in natural units, applied to q . k -- the MODEL's own (1 / sqrt(192) times a YaRN factor in the
 * checkpoints named above), not 1 / sqrt(Dk).  Required: finite and > 0, there is no default; a zero or non-finite value is
 * MFA_ERR_INVALID_ARGUMENT naming the field.  The kernel uses fl(scale x log2 e).
 *
 * cacheLengths[b] (device, uint32, required): valid keys of sequence b INCLUDING the R new tokens, which the caller has already
 * written into the cache; clamped to `column`.  The host never reads it.  The cache is never written.
 * Mask: with `causal`, row r of sequence b sees key c iff c <= r + max(cacheLengths[b] - R, 0) and c < cacheLengths[b]; without it
 * every row sees every valid key.  A sequence of length 0 gets O = 0 and L = -FLT_MAX.  Keys at or past a length, the rest of a last
 * page and pages the table does not name are never loaded: they may hold anything, NaN included.
 *
 * Layouts (strides in elements, per operand Q, KV, O):
 *   contiguous (pageSize = 0): key c of sequence b at  KV + b batchStride + c leadingDimension  (batchStride 0 shares one cache; any
 *                              row stride that is a multiple of 8 elements)
 *   paged (pageSize a power of two, 16 .. 1024): blockTable (device, int32, [batches][blockTableStride]) entry (b, i) is the page of
 *                              keys i pageSize .. (i + 1) pageSize - 1; key c lives at KV + page pageStride + (c % pageSize)
 *                              leadingDimension.  Entries past a sequence's last page are never read.
 * What the kernels need (anything else is MFA_ERR_INVALID_ARGUMENT naming the requirement; there is no slow fallback): Q and KV 16-byte
 * aligned with strides that are multiples of 8 elements; O 16-byte aligned with strides that are multiples of 4 elements; the workspace
 * 16-byte aligned.  rows <= 32 (a longer block of rows is a prefill and is not served here); heads >= 1 is otherwise free.
 *
 * Packing.  The M = heads x rows rows of a sequence are packed head-major, as decode packs a group: packed p = head x rows + row.  They
 * are cut into groups of MFA_MLA_PACKED_ROWS = 32 packed rows; one workgroup serves one group of one sequence, and one piece of its
 * keys.  A group boundary may fall inside a head's rows; the last group may be partial.
 *
 * Key pieces.  `pieces`: 0 is the host's plan, 1 is unsplit, 2 .. 64 as given, more is refused.  The plan is decode's own function
 * and constants: choose_pieces(batches x groups, the 64-key tiles of `column`, MFA_DECODE_WORKGROUP_TARGET, 4 tiles, 64 pieces).  Piece
 * s of sequence b takes mfa_attention_decode_piece_range(len_b, pieces, s).  The workspace holds pieces x batches x heads x rows x
 * (Dv + 2) x 4 bytes (the project's one formula, with D = Dv), 16-byte aligned, never assumed zeroed; nothing in it is read that the
 * launch did not write.  A NULL workspace runs unsplit and is correct; a short or misaligned one is refused in decode's words.  A piece
 * without a key publishes (m, l) = (-FLT_MAX, 0); the combine kernel reads a piece's O only where its l > 0.  With pieces a launch is a
 * straight chain of two kernels, no atomics.
 *
 * Kernels: attn_mla16_d576_<bf16|f16> (unsplit), attn_mla16_d576_<type>_k (a piece of the keys), attn_mla16_d576_<type>_combine.
 *
 * Deliberately not here: a window, sinks, a soft cap or trees on this entry; more than 32 packed rows per workgroup (at heads = 128 a
 * sequence's four groups each walk the cache); other (Dk, Dv) pairs.  In mfa_mla_cache.h, beside this header: the append kernel for the
 * latent cache, and decode over e4m3 latent caches.  In mfa_mla_prefill.h: prefill over the latent cache, blocks of rows of any length
 * (this entry still refuses rows > 32).
 */
#ifndef MFA_MLA_H
#define MFA_MLA_H

#include "mfa_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_MLA_HEAD_DIMENSION 576   /* Dk: latent + rotary */
#define MFA_MLA_VALUE_DIMENSION 512  /* Dv: the latent */
#define MFA_MLA_PACKED_ROWS 32       /* packed rows (head x rows + row) of one workgroup */

typedef struct mfa_mla_decode_params {
  uint32_t rows;                 /* R <= 32 */
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
  uint32_t pieces;               /* 0 = the host's plan, 1 = unsplit, 2 .. 64 */
  const uint32_t *cacheLengths;  /* device, [batches] */
  const int32_t *blockTable;     /* device, [batches][blockTableStride]; paged launches only */
  int64_t blockTableStride;      /* entries */
  int64_t leadingDimension[3], headStride[3], batchStride[3];   /* Q, KV, O; elements.  KV: headStride unused, batchStride contiguous only */
  int64_t pageStride;            /* KV; elements */
  int64_t lHeadStride, lBatchStride;                            /* elements of L */
  void *workspace;
  uint64_t workspaceBytes;
} mfa_mla_decode_params;

/* zeroes the block; precision = outputPrecision = MFA_BF16, headDimension = 576, valueDimension = 512, causal = 1.  scale stays 0:
 * the caller must set it */
void mfa_mla_decode_params_init(mfa_mla_decode_params *params);

/* sizeof(mfa_mla_decode_params), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_mla_decode_params_size(void);
mfa_status mfa_mla_decode_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* *bytes: what a launch in *pieces pieces needs, pieces x batches x heads x rows x (Dv + 2) x 4, 0 when the launch has one piece;
 * *pieces (may be NULL): the piece count of params->pieces -- the host's plan for 0, else as given.  The workspace the params may
 * already carry is not looked at. */
mfa_status mfa_attention_mla_decode_workspace_size(const mfa_mla_decode_params *params, uint64_t *bytes, uint32_t *pieces);

mfa_status mfa_attention_mla_decode_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                           void *stream);

/* what a launch with these parameters runs, as text: the kernels' names, the grid, the piece count */
mfa_status mfa_attention_mla_decode_launch_form(const mfa_mla_decode_params *params, char *out, size_t capacity);

/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_attention_mla_decode_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                         void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_H */
