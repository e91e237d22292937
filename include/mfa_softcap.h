/*
 * mfa_softcap.h -- C ABI of LOGIT SOFT-CAPPING over a KV cache: the decode and prefill launches of mfa_sink.h and mfa_ragged.h with
 * the attention scores passed through cap x tanh(score / cap) before the softmax (Gemma 2: attn_logit_softcapping = 50; Grok-1: 30).
 * The cap sits between Q K^T and the softmax, inside the kernel: a caller cannot apply it from outside.  An extension of mfa_sink.h,
 * whose rules hold here word for word: plain pointers and sizes, caller-owned device memory, status codes, validation before any GPU
 * call, every refusal names the requirement, asynchronous launches that copy nothing to the host and never synchronise
 * (graph-capturable).  Existing structs and entries are unchanged; the cap is one float, `softcap`, after `sinks` (after `ragged` in
 * the ragged entries) in the entries below.
 *
 * The rule.  Let raw = q . k, and s = raw x keyScale / sqrt(D) the natural-unit score the softmax sees without a cap (keyScale = 1
 * for 16-bit caches).  With softcap = cap > 0 -- natural-log units, the checkpoint's value -- the softmax sees
 *       s' = cap x tanh(s / cap)
 * instead.
 *   - The cap applies to VISIBLE scores only.  Which keys a row sees is mfa_sink.h's rule, unchanged; a masked score is replaced, never
 *     computed from: what lies past a length (NaN, 0x7f) never reaches the tanh.
 *   - The sink logit is NOT capped and not scaled.  It joins the denominator as in mfa_sink.h.
 *   - L is the log of the denominator of the CAPPED scores, plus the sink term; base-2 units, as every L of these headers.
 *   - Nothing else changes: the tiles, pages and block-table entries that are walked or never touched, the piece plan
 *     (mfa_attention_decode_sink_piece_range), the workspace size and the combine kernel, the tile ranges of prefill
 *     (mfa_attention_prefill_sink_tile_range), the slots of a ragged launch, and O = 0 / L of a row without a visible key.
 *   - Saturation: s / cap -> +-inf gives s' = +-cap, never NaN, however large the scores.
 *
 * The `softcap` argument.
 *   softcap == 0       runs exactly the launch of the header below -- mfa_sink.h with a block that has sinks, else mfa_window.h with
 *                      that window, else the plain launch; mfa_ragged.h for the ragged entries: the same kernels, launch-form text
 *                      and workspace size.
 *   softcap > 0        finite: runs the capped kernels (attn_decode16c_*, attn_decode8c_*, attn_prefill16c_*[_e4m3], and
 *                      attn_prefill16rc_*[_e4m3] over packed rows) WHATEVER the window and sinks: one family, the sink kernels plus the
 *                      cap.  The workspace size equals the sink launch's of the same window and sinks.
 *   negative, NaN, inf MFA_ERR_INVALID_ARGUMENT.
 *
 * `sinks` may be NULL in these entries: no sinks (as in mfa_ragged.h).  `window` 0: no window; `quant` NULL: a 16-bit cache.
 */
#ifndef MFA_SOFTCAP_H
#define MFA_SOFTCAP_H

#include "mfa_ragged.h"
#include "mfa_sink.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the decode entries of mfa_sink.h with `softcap` after `sinks` (NULL: none) */
mfa_status mfa_attention_decode_softcap_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                       const mfa_attention_sinks *sinks, float softcap, uint64_t *bytes);
mfa_status mfa_attention_decode_softcap_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                               const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                               const mfa_attention_sinks *sinks, float softcap, void *stream);
mfa_status mfa_attention_decode_softcap_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                    const mfa_attention_sinks *sinks, float softcap, char *out, size_t capacity);
mfa_status mfa_attention_decode_softcap_time(const void *q, const void *k, const void *v, void *o, float *l,
                                             const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                             const mfa_attention_sinks *sinks, float softcap, void *stream, int warmup, int iterations,
                                             float *milliseconds);

/* the prefill entries of mfa_sink.h with `softcap` after `sinks` (NULL: none) */
mfa_status mfa_attention_prefill_softcap_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                                const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                float softcap, void *stream);
mfa_status mfa_attention_prefill_softcap_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                     float softcap, char *out, size_t capacity);
mfa_status mfa_attention_prefill_softcap_time(const void *q, const void *k, const void *v, void *o, float *l,
                                              const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                              float softcap, void *stream, int warmup, int iterations, float *milliseconds);

/* the prefill entries of mfa_ragged.h with `softcap` after `ragged` (required, as there) */
mfa_status mfa_attention_prefill_ragged_softcap_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                                       const mfa_prefill_params *params, uint32_t window,
                                                       const mfa_attention_sinks *sinks, const mfa_ragged_rows *ragged, float softcap,
                                                       void *stream);
mfa_status mfa_attention_prefill_ragged_softcap_launch_form(const mfa_prefill_params *params, uint32_t window,
                                                            const mfa_attention_sinks *sinks, const mfa_ragged_rows *ragged,
                                                            float softcap, char *out, size_t capacity);
mfa_status mfa_attention_prefill_ragged_softcap_time(const void *q, const void *k, const void *v, void *o, float *l,
                                                     const mfa_prefill_params *params, uint32_t window,
                                                     const mfa_attention_sinks *sinks, const mfa_ragged_rows *ragged, float softcap,
                                                     void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_SOFTCAP_H */
