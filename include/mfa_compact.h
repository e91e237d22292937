/*
 * mfa_compact.h -- C ABI of the COMPACTION of the accepted speculation-tree path inside a KV cache: the launch that closes the loop
 * append -> verify -> accept -> continue of mfa_tree.h.  mfa_kv_cache_append_launch wrote the R nodes of a draft tree into the slots
 * P .. P + R - 1 of every sequence and a tree launch verified them; the engine then accepts ONE root-to-leaf path, whose nodes sit
 * scattered among their rejected siblings.  This launch moves the K and V rows of the accepted nodes to the slots P, P + 1, ... in
 * place and says what the sequence's length has become, so that the next step appends behind them.  An extension of mfa_tree.h, whose
 * rules hold here word for word: plain pointers and sizes, caller-owned device memory, status codes, validation before any GPU call,
 * every refusal names the requirement, an asynchronous launch that copies nothing to the host and never synchronises
 * (graph-capturable).  Existing structs and entries are unchanged.
 *
 * The rule, in the vocabulary of mfa_tree.h.  For sequence b:
 *       n    = min(cacheLengths[b], column)           (a paged cache: cacheLengths[b]; the page rules below bound it)
 *       qn   = rows, or min(queryLengths[b], rows) when queryLengths is given       (the tree rows)
 *       P    = max(n - qn, 0),  live = min(qn, n)                                   (node j sits at key P + j, j < live)
 *       a    = min(acceptedCounts[b], maxAccepted, live)
 * `accepted`: device int32 [batches][acceptedStride], node indices in PATH order, root first; `acceptedCounts`: device uint32 [batches].
 * For every K/V head, for K and for V, and for i < a with j = accepted[b x acceptedStride + i]:
 *       the row at key P + i becomes the row that stood at key P + j BEFORE THE LAUNCH.
 * These are GATHER semantics: every source is read before any destination is written.  The indices need not increase -- mfa_tree.h
 * honours bits j > r, so a child may have a smaller index than its parent: a rotation or a reversal is a legal path, and repeated
 * indices are well defined.
 *
 * Dropped rows.  An index j < 0 or j >= live drops row i: nothing is read and nothing is written.  A paged row whose source or
 * destination page index is >= blockTableStride, or whose table entry is negative, is dropped in the same way -- the drop rules of
 * mfa_kv_cache_append_launch.
 *
 * What else the launch does.  newLengths[b] = P + a goes to a separate device array of uint32 [batches] (NULL: not wanted).  It is
 * refused when its range overlaps cacheLengths: other workgroups still read the old length.  No other byte of the cache, the pool, the
 * tables or the scales changes; a row that is already in place (j = i) may be skipped.  An e4m3 cache is moved as bytes: scales are per
 * head and do not enter.  The host reads no device array.
 *
 * Caches.  The layouts of mfa_kv_cache_append_launch: contiguous with strides (token-major included), or paged (pageSize a power of
 * two 16 .. 1024, K and V share the table); MFA_FP16 / MFA_BF16 elements or MFA_KV_E4M3 bytes; head dimensions 64, 128 and 256.  Both
 * buffers 16-byte aligned; strides of a 16-bit cache multiples of 8 elements, of an e4m3 cache multiples of 16.
 *
 * Refused before any GPU call, in this order: null params; a cachePrecision that is neither 16-bit nor e4m3 (e5m2: MFA_ERR_UNSUPPORTED);
 * a head dimension outside 64 / 128 / 256; zero rows, heads or batches, or 2 x heads x batches above the 2^31 - 1 workgroups of a grid;
 * rows or maxAccepted above MFA_TREE_MAX_NODES, or maxAccepted 0; acceptedStride < maxAccepted; NULL cacheLengths, accepted or
 * acceptedCounts; misaligned accepted; newLengths overlapping cacheLengths, or misaligned; the paging and stride errors in the words
 * of the append launch; null or misaligned cache buffers.
 *
 * Kernels: kv_cache_compact_b64 / _b128 / _b256 / _b512, one per byte count of a row, which is all that matters to a move -- bf16, f16
 * and e4m3 share them.  One workgroup per (sequence, K or V, K/V head) loads the a rows of its slab into registers, 16 bytes at a
 * time, passes a workgroup barrier and stores them: slabs of different workgroups are disjoint.
 */
#ifndef MFA_COMPACT_H
#define MFA_COMPACT_H

#include "mfa_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfa_kv_compact_params {
  uint32_t rows;                  /* R tree rows per sequence, <= MFA_TREE_MAX_NODES */
  uint32_t heads;                 /* K / V heads */
  uint32_t batches;
  uint32_t column;                /* capacity (keys) of a contiguous cache */
  uint16_t headDimension;
  uint8_t cachePrecision;         /* MFA_FP16 / MFA_BF16, or MFA_KV_E4M3 */
  uint8_t reserved;               /* 0 */
  uint32_t pageSize;              /* 0 = contiguous */
  const uint32_t *cacheLengths;   /* device, [batches]; includes the tree rows (what the append and the tree launch took) */
  const uint32_t *queryLengths;   /* device, [batches]; NULL = `rows` for every sequence */
  const int32_t *blockTable;      /* device, [batches][blockTableStride]; paged only */
  int64_t blockTableStride;
  const int32_t *accepted;        /* device, [batches][acceptedStride]: node indices in path order, root first; 4-byte aligned */
  int64_t acceptedStride;         /* elements between two sequences' paths, >= maxAccepted */
  const uint32_t *acceptedCounts; /* device, [batches] */
  uint32_t maxAccepted;           /* 1 .. MFA_TREE_MAX_NODES: the most rows a sequence moves */
  uint32_t reserved2;             /* 0 */
  uint32_t *newLengths;           /* device, [batches]: P + a; NULL = not wanted; must not overlap cacheLengths */
  int64_t leadingDimension[2], headStride[2], batchStride[2];   /* kCache, vCache; elements.  batchStride: contiguous only */
  int64_t pageStride[2];          /* kCache, vCache; elements */
} mfa_kv_compact_params;

/* zeroes the block; cachePrecision = MFA_BF16 */
void mfa_kv_compact_params_init(mfa_kv_compact_params *params);

/* sizeof(mfa_kv_compact_params), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity`
 * are written): what a binding's mirror of the struct is checked against */
size_t mfa_kv_compact_params_size(void);
mfa_status mfa_kv_compact_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

mfa_status mfa_kv_cache_compact_launch(void *kCache, void *vCache, const mfa_kv_compact_params *params, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MFA_COMPACT_H */
