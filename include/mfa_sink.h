/*
 * mfa_sink.h -- C ABI of ATTENTION SINKS over a KV cache: the decode and prefill launches of mfa_window.h with sink TOKENS (the first
 * keys of a sequence stay visible to every row however far its window has moved on: StreamingLLM-style serving) and sink LOGITS (one
 * learned logit per query head that joins the softmax denominator and no value row: every gpt-oss layer).  An extension of
 * mfa_window.h, whose rules hold here word for word: plain pointers and sizes, caller-owned device memory, status codes, validation
 * before any GPU call, every refusal names the requirement, asynchronous launches that copy nothing to the host and never
 * synchronise (graph-capturable).  Existing structs and entries are unchanged; the sinks are one small block, mfa_attention_sinks,
 * after `window` in the entries below.
 *
 * The rule.  With n, qn, the frontier f(r), lim(r) = min(n, f + 1) and lo(r) = max(f + 1, W) - W exactly as in mfa_window.h (window
 * W = 0: lo = 0 everywhere), two independent options:
 *
 *   sinkTokens = S (0 = none; needs a window W >= 1 and `causal`, otherwise MFA_ERR_INVALID_ARGUMENT).  Row r sees key c iff
 *       c < lim(r)   and   (c >= lo(r)   or   c < S):
 *     the window plus the keys [0, min(S, lim)).  S may exceed n or reach into the window: both are just the union.
 *
 *   sinkLogits (device float[heads], one per QUERY head; NULL = none; any window, 0 included; `causal` not required).  Natural-log
 *     units, the checkpoint's value: it is NOT multiplied by 1 / sqrt(D) or by an e4m3 cache's key scale.  With s2 = sink log2(e),
 *     m the largest base-2 score of the row and l = sum 2^(score - m):
 *       O = sum p v / (l + 2^(s2 - m)),     L = m + log2(l + 2^(s2 - m))      (base-2 units, as every L of these headers)
 *     -- L includes the sink, so that a later merge of two states stays correct.  A live row without a visible key gets O = 0 and
 *     L = s2 (without logits it stays -FLT_MAX).  The values must be finite; the host never reads them.  No probability mass is added
 *     to any V row.
 *
 * A block with sinkTokens = 0 and sinkLogits = NULL runs exactly the mfa_window.h launch of the same `window`: the same kernels,
 * launch-form text and workspace size.  Anything else runs the sink kernels (attn_decode16s_*, attn_decode8s_*, attn_prefill16s_*):
 * the window kernels plus the two options.
 *
 * What is never loaded.  Keys at or past n, as before.  With sink tokens a launch walks TWO disjoint ranges of 64-key tiles, the sink
 * tiles [0, sinkTiles) and the window's tiles; the keys in the tiles between them (at or past sinkTiles and below the window's first
 * tile), the pages that hold only such keys and their block-table entries are never loaded: they may hold anything, NaN or 0x7f
 * included, the entries may be stale -- an engine frees exactly those pages.  blockTable stays indexed by ABSOLUTE page number.
 * Inside a walked tile, keys a row does not see are loaded and masked (their score is replaced, p = 0 exactly): they must be finite.
 *
 * Decode.  With lo0, first = lo0 / 64 and last = ceil(n / 64) as in mfa_window.h, sinkTiles = min(ceil(min(S, n) / 64), first); the
 * launch walks the tile LIST [0, sinkTiles) ++ [first, last) and cuts that list into pieces
 * (mfa_attention_decode_sink_piece_range): a piece is at most two key ranges.  Piece 0 folds the sink logit into the (m, l) it
 * publishes (an empty piece 0: m = s2, l = 1, O = 0), so the combine kernel of mfa_decode.h merges the pieces as it stands.  The host
 * plans the piece count from min(column's tiles, the window's bound + ceil(S / 64)) tiles.
 *
 * Prefill.  A row block walks the tiles [0, sinkEnd) and then [begin, end) of mfa_attention_prefill_sink_tile_range, nothing else.
 */
#ifndef MFA_SINK_H
#define MFA_SINK_H

#include "mfa_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfa_attention_sinks {
  uint32_t sinkTokens;       /* S: the first S keys stay visible under the window; 0 = none */
  uint32_t reserved;         /* 0 */
  const float *sinkLogits;   /* device, [heads] (query heads), natural-log units; NULL = none */
} mfa_attention_sinks;

/* zeroes the block: no sink tokens, no sink logits */
void mfa_attention_sinks_init(mfa_attention_sinks *sinks);

/* sizeof(mfa_attention_sinks), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_attention_sinks_size(void);
mfa_status mfa_attention_sinks_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* the decode entries of mfa_window.h with `sinks` after `window` (`quant` NULL: a 16-bit cache; `window` 0: no window).  `sinks` is
 * required: a NULL block is refused, an all-zero one is the mfa_window.h launch */
mfa_status mfa_attention_decode_sink_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                    const mfa_attention_sinks *sinks, uint64_t *bytes);
mfa_status mfa_attention_decode_sink_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                            const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                            const mfa_attention_sinks *sinks, void *stream);
mfa_status mfa_attention_decode_sink_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                 const mfa_attention_sinks *sinks, char *out, size_t capacity);
mfa_status mfa_attention_decode_sink_time(const void *q, const void *k, const void *v, void *o, float *l,
                                          const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                          const mfa_attention_sinks *sinks, void *stream, int warmup, int iterations, float *milliseconds);

/* the kernels' own piece function, on the host (rows >= 1; window 0: no window, which admits no sink tokens).  The walked tile list
 * is [0, sinkTiles) ++ [first, last) as above; piece `piece` of `pieces` takes an equal share, in whole tiles, of that LIST: the
 * keys [begin[0], end[0]) of the sink tiles and [begin[1], end[1]) of the window's tiles.  Either may be empty (begin == end); both are
 * clamped to `length` as mfa_attention_decode_piece_range clamps.  With sinkTokens = 0 the first range is empty and the second is
 * mfa_attention_decode_window_piece_range's.  The unsplit kernel runs it with pieces = 1. */
mfa_status mfa_attention_decode_sink_piece_range(uint32_t length, uint32_t rows, uint32_t window, uint32_t sinkTokens, uint32_t pieces,
                                                 uint32_t piece, uint32_t begin[2], uint32_t end[2]);

/* the prefill entries of mfa_window.h with `sinks` after `window` */
mfa_status mfa_attention_prefill_sink_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                             const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                             void *stream);
mfa_status mfa_attention_prefill_sink_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                  char *out, size_t capacity);
mfa_status mfa_attention_prefill_sink_time(const void *q, const void *k, const void *v, void *o, float *l,
                                           const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                           void *stream, int warmup, int iterations, float *milliseconds);

/* the kernels' own tile-range function, on the host.  For the block of rows [firstRow, firstRow + blockRows) of a sequence of `length`
 * keys and `queryLength` rows, in 64-key tiles: the four indices of mfa_attention_prefill_window_tile_range (window 0: begin =
 * unmaskedBegin = 0 and mfa_attention_prefill_tile_range's two under `causal`), plus *sinkEnd = min(ceil(min(S, lim(last live row))
 * / 64), *begin): the tiles [0, *sinkEnd) are walked first, always with the per-element mask, then [*begin, *end); no other tile is
 * loaded.  A block whose rows all lie past their window's keys (length < queryLength) still sees its sink keys: begin = unmaskedBegin
 * = unmaskedEnd = end = sinkEnd = ceil(min(S, length) / 64).  A block without a live row or without a visible key: all five 0.
 * A window and sink tokens need `causal`; sink tokens need a window. */
mfa_status mfa_attention_prefill_sink_tile_range(uint32_t length, uint32_t queryLength, uint32_t firstRow, uint32_t blockRows,
                                                 uint32_t causal, uint32_t window, uint32_t sinkTokens, uint32_t *begin,
                                                 uint32_t *unmaskedBegin, uint32_t *unmaskedEnd, uint32_t *end, uint32_t *sinkEnd);

#ifdef __cplusplus
}
#endif
#endif /* MFA_SINK_H */
