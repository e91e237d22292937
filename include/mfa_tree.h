/*
 * mfa_tree.h -- C ABI of SPECULATION TREES over a KV cache: the decode and prefill launches of mfa_sink.h with the new rows of a
 * sequence taken as the nodes of a draft TREE (Medusa, EAGLE, SpecInfer and their descendants) instead of a chain.  A node sees the
 * cached prefix and its own ancestors; it does not see its siblings, which sit in neighbouring cache slots.  The rule sits between
 * Q K^T and the softmax, inside the kernel: from outside, a caller can only launch once per root-to-leaf path and re-read the cache
 * every time.  An extension of mfa_sink.h, whose rules hold here word for word: plain pointers and sizes, caller-owned device memory,
 * status codes, validation before any GPU call, every refusal names the requirement, asynchronous launches that copy nothing to the
 * host and never synchronise (graph-capturable).  Existing structs and entries are unchanged; the tree is one small block,
 * mfa_attention_tree, after `sinks` in the entries below.  The draft tokens are appended with mfa_kv_cache_append_launch as ever.
 *
 * The rule.  For sequence b, with n = min(cacheLengths[b], column) and qn its new rows (decode: `rows`; prefill: min(queryLengths[b],
 * rows)): P = max(n - qn, 0) is the prefix length, the new tokens are the keys P .. n - 1, node j at key P + j, and live = min(qn, n).
 *       mask_r = masks[b x batchStride + r] & (2^live - 1)         (bits at or past `live` are ignored)
 *       d_r    = max(popcount(mask_r), 1)                           (the node's depth + 1: a well-formed mask holds the node's ancestors
 *                                                                    and the node itself)
 * Row r sees key c iff one of these holds:
 *   - PREFIX key: c < P, and either there is no window, or c >= max(P + d_r, W) - W, or c < S.  This is mfa_sink.h's window and sink
 *     rule with the row's frontier at its POSITION P + d_r - 1, not at its index.
 *   - NEW-TOKEN key: P <= c < n and bit (c - P) of mask_r is set.  The mask alone decides: no causal test and no window test among the
 *     new tokens, and bits j > r are honoured.
 * Unchanged: a masked score is replaced, never computed from; a row without a visible key keeps O = 0 and L = -FLT_MAX, or the sink
 * logit; sink logits and the K / V scales; what is never loaded.  The chain mask_r = 2^(r + 1) - 1 gives d_r = r + 1 and, with W >= rows,
 * the visible set of the mfa_sink.h launch for every (n, qn, W, S), n < qn included: the tree launch is then that launch bit for bit.
 *
 * The block.  `masks`: device array of uint64, 8-byte aligned, [batches][rows]; `batchStride` in elements, 0 = one tree shared by every
 * sequence (a static topology).  The host never reads the masks.  Trees that differ in size per sequence: queryLengths (prefill).
 *
 * Refused before any GPU call: causal = 0 (a tree needs the causal launch, as a window does); 0 < window < rows (an ancestor could fall
 * outside a descendant's window; with W >= rows it never does); prefill rows > MFA_TREE_MAX_NODES (one uint64 per row; decode keeps
 * headsPerKeyValue x rows <= 32); NULL or misaligned masks; a NULL `tree`.  A soft cap or packed rows (mfa_softcap.h, mfa_ragged.h)
 * together with a tree have no kernel and no entry.
 *
 * Decode.  Nothing but the rule changes: the piece plan (mfa_attention_decode_sink_piece_range with `rows` -- row 0's frontier P + 1 is
 * the smallest a node can have), the workspace size and the combine kernel are the sink launch's.  Kernels: attn_decode16t_*,
 * attn_decode8t_*.
 *
 * Prefill.  A row's mask may name any new token and its depth is not its index, so EVERY row block of a sequence walks the same
 * tiles: [0, sinkEnd) and then [begin, end) of mfa_attention_prefill_tree_tile_range, nothing else.  Kernels: attn_prefill16t_*[_e4m3].
 */
#ifndef MFA_TREE_H
#define MFA_TREE_H

#include "mfa_sink.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_TREE_MAX_NODES 64u /* rows of a prefill launch with a tree: one bit of a mask each */

typedef struct mfa_attention_tree {
  const uint64_t *masks; /* device, [batches][rows]: bit j of masks[b x batchStride + r] = row r sees node j; 8-byte aligned */
  int64_t batchStride;   /* elements between two sequences' masks; 0 = one tree shared by every sequence */
  uint64_t reserved;     /* 0 */
} mfa_attention_tree;

/* zeroes the block (masks must then be set) */
void mfa_attention_tree_init(mfa_attention_tree *tree);

/* sizeof(mfa_attention_tree), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_attention_tree_size(void);
mfa_status mfa_attention_tree_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* the decode entries of mfa_sink.h with `tree` after `sinks` (`quant` NULL: a 16-bit cache; `window` 0: no window; `sinks` NULL: none).
 * `tree` is required */
mfa_status mfa_attention_decode_tree_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                    const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, uint64_t *bytes);
mfa_status mfa_attention_decode_tree_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                            const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                            const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, void *stream);
mfa_status mfa_attention_decode_tree_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                 const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, char *out,
                                                 size_t capacity);
mfa_status mfa_attention_decode_tree_time(const void *q, const void *k, const void *v, void *o, float *l,
                                          const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                          const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, void *stream, int warmup,
                                          int iterations, float *milliseconds);

/* the prefill entries of mfa_sink.h with `tree` after `sinks` (NULL: none).  `tree` is required */
mfa_status mfa_attention_prefill_tree_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                             const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                             const mfa_attention_tree *tree, void *stream);
mfa_status mfa_attention_prefill_tree_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                  const mfa_attention_tree *tree, char *out, size_t capacity);
mfa_status mfa_attention_prefill_tree_time(const void *q, const void *k, const void *v, void *o, float *l,
                                           const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                           const mfa_attention_tree *tree, void *stream, int warmup, int iterations, float *milliseconds);

/* the kernels' own tile-range function, on the host: the 64-key tiles EVERY row block of a sequence of `length` keys and `queryLength`
 * rows walks (it does not depend on the row block).  With P, live as above and lo(f) = window ? max(f, window) - window : 0:
 *   *begin = floor(lo(P + 1) / 64), *end = ceil(length / 64);
 *   [*unmaskedBegin, *unmaskedEnd) = [ceil(lo(P + live) / 64), floor(P / 64)) run without the per-element mask -- every key of theirs
 *   is a prefix key inside every row's window; key P is a tree key and masked; an empty range: both = *begin;
 *   *sinkEnd = min(ceil(min(sinkTokens, P) / 64), *begin): the tiles [0, *sinkEnd) are walked first, with the per-element mask.
 * length = 0 or queryLength = 0: all five 0.  Sink tokens need a window. */
mfa_status mfa_attention_prefill_tree_tile_range(uint32_t length, uint32_t queryLength, uint32_t window, uint32_t sinkTokens,
                                                 uint32_t *begin, uint32_t *unmaskedBegin, uint32_t *unmaskedEnd, uint32_t *end,
                                                 uint32_t *sinkEnd);

#ifdef __cplusplus
}
#endif
#endif /* MFA_TREE_H */
