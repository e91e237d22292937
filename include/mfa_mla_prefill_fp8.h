/*
 * mfa_mla_prefill_fp8.h -- C ABI of multi-head latent attention PREFILL over an E4M3 latent cache, unsplit and cut along the keys: the
 * launches of mfa_mla_prefill.h and mfa_mla_prefill_split.h over the cache mfa_mla_cache.h's append kernel writes and its decode reads,
 * so that an FP8 latent cache is usable end to end (append -> prefill -> decode) without a 16-bit copy.  The "e4m3 latent caches" those
 * three headers name as not built live HERE: they, their structs and their entries are unchanged and run what they ran.  Their rules
 * hold word for word: plain pointers and sizes, caller-owned device memory, status codes, validation before any GPU call, every refusal
 * names the requirement, asynchronous launches that copy nothing to the host and never synchronise (graph-capturable: one kernel, or a
 * straight chain of two; no atomics, no host reads).
 *
 * No new struct.  A launch takes mfa_mla_prefill_params unchanged, mfa_mla_quant (mfa_mla_cache.h: cachePrecision = MFA_KV_E4M3;
 * kvScale a device pointer to ONE FP32, NULL = 1.0, never read by the host) and, cut, mfa_key_split (mfa_split.h), as they are.
 * Q, O, L, the mask with queryLengths, the row-major packing p = row x heads + head, the blocks of 64,
 * mfa_attention_mla_prefill_step_range, "rows at or past queryLengths[b] are neither read nor written" and "a row without a visible key
 * gets O = 0 and L = -FLT_MAX" are mfa_mla_prefill.h's.  Three things differ:
 *
 * The cache is mfa_mla_cache.h's e4m3 format: one row of 576 BYTES a key (512 latent, 64 rotary), contiguous or paged.  The KV strides
 * are in elements = bytes and are multiples of 16; the cache pointer is 16-byte aligned.  `precision` stays the 16-bit type of Q.  A
 * stored byte b stands for kvScale[0] x e4m3(b).
 *
 * What is never loaded: keys at or past n = min(cacheLengths[b], column), the rest of a last page, pages that no table names and table
 * entries past the last page.  They may hold anything, the NaN bytes 0x7f / 0xff included.
 *
 * The scale folds as in decode over the e4m3 cache: the score scale is fl(fl(scale x log2 e) x kvScale); the unsplit launch's last
 * multiplication is by fl(fl(1 / l) x kvScale); a piece publishes fl(o x kvScale) un-normalised, so the combine arithmetic is
 * mfa_mla_prefill_split.h's, unchanged.  For every packed row the arithmetic is that of mfa_attention_mla_decode_fp8_launch at one
 * piece, bit for bit: a row's result depends neither on its block nor on how a prompt is cut into launches.
 *
 * The cut launch.  The piece plan (pieces = 0), mfa_attention_mla_prefill_split_piece_range and the workspace formula are
 * mfa_mla_prefill_split.h's own: bytes and pieces equal mfa_attention_mla_prefill_split_workspace_size's for the same params and
 * split.  A NULL workspace, or one piece, IS the unsplit fp8 launch (the launch form says "unsplit without a workspace: the plan has N
 * pieces").
 *
 * Refusals, in this order: a NULL quant block; a cachePrecision other than MFA_KV_E4M3 (MFA_KV_E5M2 is MFA_ERR_UNSUPPORTED);
 * quant.reserved != 0; a KV leading dimension, batch stride or page stride that is not a multiple of 16; for the cut entries
 * everything mfa_mla_prefill_split.h refuses about `split`, in its words; everything mfa_mla_prefill.h refuses about the params, in its
 * words; a short or misaligned workspace, naming mfa_attention_mla_prefill_fp8_split_workspace_size; Q, KV or O NULL or not 16-byte
 * aligned, L or kvScale not 4-byte aligned.
 *
 * Kernels: attn_mla8p_d576_<bf16|f16> (unsplit), attn_mla8pk_d576_<type> (a piece), attn_mla8p_d576_<type>_combine.
 *
 * Deliberately not here: ragged (packed-axis) rows, lists of key positions, a window, sinks, a soft cap or trees under MLA prefill;
 * per-token or per-128-column scales (the 656-byte layout included); e5m2; an FP8 Q or the FP8 matrix instructions; the split as the
 * default of the torch binding (key_pieces = 1 unless asked).
 */
#ifndef MFA_MLA_PREFILL_FP8_H
#define MFA_MLA_PREFILL_FP8_H

#include "mfa_mla_cache.h"
#include "mfa_mla_prefill_split.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the entries of mfa_mla_prefill.h with `quant` after `params`.  `quant` is required */
mfa_status mfa_attention_mla_prefill_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                const mfa_mla_quant *quant, void *stream);
mfa_status mfa_attention_mla_prefill_fp8_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_quant *quant, char *out,
                                                     size_t capacity);
mfa_status mfa_attention_mla_prefill_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                              const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds);

/* the entries of mfa_mla_prefill_split.h with `quant` after `split`.  Both are required */
mfa_status mfa_attention_mla_prefill_fp8_split_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                      const mfa_key_split *split, const mfa_mla_quant *quant, void *stream);
mfa_status mfa_attention_mla_prefill_fp8_split_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                           const mfa_mla_quant *quant, char *out, size_t capacity);
mfa_status mfa_attention_mla_prefill_fp8_split_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                    const mfa_key_split *split, const mfa_mla_quant *quant, void *stream, int warmup,
                                                    int iterations, float *milliseconds);
/* *bytes and *pieces (may be NULL) as mfa_attention_mla_prefill_split_workspace_size gives them; the workspace `split` may already
 * name is not looked at */
mfa_status mfa_attention_mla_prefill_fp8_split_workspace_size(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                              const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_PREFILL_FP8_H */
