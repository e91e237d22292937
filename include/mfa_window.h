/*
 * mfa_window.h -- C ABI of SLIDING-WINDOW attention over a KV cache: the decode and prefill launches of mfa_decode.h, mfa_kvcache.h
 * and mfa_prefill.h with a window of `window` keys behind every row's causal frontier (the local layers of Mistral, Gemma 2 / 3,
 * gpt-oss).  An extension of those headers, whose rules hold here word for word: plain pointers and sizes, caller-owned device
 * memory, status codes, validation before any GPU call, every refusal names the requirement, asynchronous launches that copy
 * nothing to the host and never synchronise (graph-capturable).  Their structs and entries are unchanged; the window is one plain
 * `uint32_t window` argument of the entries below.
 *
 * The rule.  With n = min(cacheLengths[b], column), qn = queryLengths[b] (decode: qn = rows) and the frontier of row r
 * f(r) = r + max(n - qn, 0), row r sees key c iff
 *     c < n   and   c <= f(r)   and   c + window > f(r):
 * itself and the window - 1 keys before it, `window_size = (window - 1, 0)` elsewhere.  A window needs `causal`: without it the
 * launch returns MFA_ERR_INVALID_ARGUMENT.  A live row without a visible key (possible when n < qn) gets O = 0 and L = -FLT_MAX.
 *
 * window = 0 means NO window: such an entry runs exactly the launch of the header it extends -- the same kernels, the same
 * launch-form text, the same workspace size.  Only 0 does that: any other window, however large, runs the window kernels
 * (attn_decode16w_*, attn_decode8w_*, attn_prefill16w_*), which with window >= column + rows compute the plain launch's values
 * in the plain launch's order, byte for byte.
 *
 * What is never loaded.  Keys at or past n, as before.  And keys below the first 64-key tile that any row of the workgroup sees,
 * the pages that hold only such keys and their block-table entries are never loaded: they may hold anything, NaN or 0x7f
 * included -- an engine may free the pages that fell out of the window and leave their table entries stale.  blockTable is still
 * indexed by ABSOLUTE page number (entry i names the page of keys i pageSize ..), and blockTableStride must still hold the pages
 * of `column` keys.  Inside the first tile a workgroup loads, keys below a row's window are loaded and masked (their score is
 * replaced, p = 0 exactly): they must hold finite values, as the keys between a causal frontier and n always had to.
 *
 * Decode.  The first key any row of a sequence sees is lo0 = max(max(n - rows, 0) + 1, window) - window; the launch walks the tiles
 * [lo0 / 64, ceil(n / 64)) and cuts THOSE into pieces (mfa_attention_decode_window_piece_range; pieces may be empty, the combine
 * kernel of mfa_decode.h merges them as it stands).  The host knows only `column`: a windowed sequence walks at most
 * ceil((window + rows - 1) / 64) + 1 tiles, and the piece count is chosen from the smaller of that and column's tiles -- so the
 * workspace a windowed launch wants shrinks with the window.  `quant` = NULL is a 16-bit cache, otherwise the e4m3 cache's block:
 * one set of entries serves both.
 *
 * Prefill.  A row block walks the tiles [begin, end) of mfa_attention_prefill_window_tile_range and nothing else.
 */
#ifndef MFA_WINDOW_H
#define MFA_WINDOW_H

#include "mfa_prefill.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the entries of mfa_kvcache.h's decode over an e4m3 cache, with `window` after `quant` (NULL: a 16-bit cache) */
mfa_status mfa_attention_decode_window_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                      uint64_t *bytes);
mfa_status mfa_attention_decode_window_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                              const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window, void *stream);
mfa_status mfa_attention_decode_window_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window, char *out,
                                                   size_t capacity);
mfa_status mfa_attention_decode_window_time(const void *q, const void *k, const void *v, void *o, float *l,
                                            const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window, void *stream,
                                            int warmup, int iterations, float *milliseconds);

/* the kernels' own piece function, on the host (window >= 1).  With lo0 as above, piece `piece` of `pieces` takes an equal share,
 * in whole tiles, of the tiles [lo0 / 64, ceil(length / 64)); *end is clamped to `length` and *begin to *end, as
 * mfa_attention_decode_piece_range does.  The unsplit kernel runs it with pieces = 1. */
mfa_status mfa_attention_decode_window_piece_range(uint32_t length, uint32_t rows, uint32_t window, uint32_t pieces, uint32_t piece,
                                                   uint32_t *begin, uint32_t *end);

/* the entries of mfa_prefill.h with `window` after `params` */
mfa_status mfa_attention_prefill_window_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                               const mfa_prefill_params *params, uint32_t window, void *stream);
mfa_status mfa_attention_prefill_window_launch_form(const mfa_prefill_params *params, uint32_t window, char *out, size_t capacity);
mfa_status mfa_attention_prefill_window_time(const void *q, const void *k, const void *v, void *o, float *l,
                                             const mfa_prefill_params *params, uint32_t window, void *stream, int warmup, int iterations,
                                             float *milliseconds);

/* the kernels' own tile-range function, on the host (window >= 1, causal).  For the block of rows [firstRow, firstRow + blockRows)
 * of a sequence of `length` keys and `queryLength` rows, in 64-key tiles: tiles outside [*begin, *end) are never loaded;
 * [*unmaskedBegin, *unmaskedEnd) is exactly the set of tiles in which every key is visible to every live row of the block (they run
 * without the per-element mask); an empty set is unmaskedBegin == unmaskedEnd inside [begin, end].  A block without a live row or
 * without a visible key: all four 0. */
mfa_status mfa_attention_prefill_window_tile_range(uint32_t length, uint32_t queryLength, uint32_t firstRow, uint32_t blockRows,
                                                   uint32_t window, uint32_t *begin, uint32_t *unmaskedBegin, uint32_t *unmaskedEnd,
                                                   uint32_t *end);

#ifdef __cplusplus
}
#endif
#endif /* MFA_WINDOW_H */
