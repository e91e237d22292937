/*
 * mfa_mla_prefill_sparse.h -- C ABI of SPARSE multi-head latent attention PREFILL: the launch of mfa_mla_prefill.h over a per-row list
 * of selected keys instead of over every key below the frontier -- the prompt chunk of DeepSeek-V3.2, whose indexer picks 2048 keys per
 * query token, shared by all heads, out of the same 576-wide latent cache.  Two existing blocks, both UNCHANGED: mfa_mla_prefill_params
 * (Q, the cache and its layouts, O, L, scale, cacheLengths, queryLengths, causal, any number of rows, precision: all as there, a 16-bit
 * cache) and beside it mfa_mla_sparse (mfa_mla_sparse.h), passed the way the sparse decode takes it.  No existing struct or entry
 * changes; there is no workspace.
 *
 *   indices  [batches][rows][topk]  int32, device: the list of row r of sequence b starts at indices + b indexBatchStride +
 *            r indexRowStride and has `topk` slots; every head of that row attends to the same list.  Strides and alignment are
 *            mfa_mla_sparse's: 4-byte aligned, indexRowStride >= topk, indexBatchStride 0 shares one set of lists.
 *
 * What an entry is.  indices[b][r][j] is a key POSITION c of sequence b: a logical position; a paged launch translates it through the
 * block table exactly as the dense launch does.
 * When a slot is visible.  Prefill's rule over a list: with n = min(cacheLengths[b], column) and qn = min(queryLengths[b], rows), slot j
 * of row r < qn is visible iff 0 <= c < n and, with `causal`, c <= r + max(n - qn, 0).
 * Holes.  Any other value is a hole, anywhere in the list: -1, entries below -1, a position at or past n, a position past the causal
 * frontier, and the slots of a last partial step of 32.  Its score is replaced, never computed from; its cache row is NEVER LOADED; its
 * block-table entry is never read.  Nothing past slot topk - 1 of a list is read.
 * What is never loaded.  A key that no list of the launch names is never loaded either: such rows, pages and table entries may hold
 * anything, NaN included.  Rows at or past queryLengths[b] are neither read (Q, their lists) nor written (O, L).
 * Repeated positions.  A position that appears twice in a list COUNTS TWICE.  Callers pass distinct positions.
 * Empty rows.  A row r < qn with no visible slot gets O = 0 and L = -FLT_MAX.
 * Device reads.  The host reads neither the lists nor a length: one capture in a graph serves changed lists and lengths.
 *
 * Packing.  The rows packed into one workgroup must share one list, so a workgroup serves 32 HEADS of ONE (sequence, row):
 * head = 32 group + q, groups = ceil(heads / 32); the grid is batches x rows x groups, group fastest, so that the groups of one
 * (sequence, row) -- which gather the same cache rows -- are neighbours.  Lanes of heads at or past `heads` repeat the last head and
 * store nothing.  A workgroup whose row is at or past queryLengths[b] returns at once.  (A workgroup of 64 heads as two tiles of 32
 * against one gather was built and measured: 1.3 x slower at heads = 128.  It exists only under -DMFA_MLAPX_TWO_TILES.)
 *
 * For every row the arithmetic is that of mfa_mla_sparse.h's unsplit kernel, bit for bit: a row's result does not depend on how a
 * prompt is cut into launches, and with the list 0 .. column - 1 it is mfa_mla_prefill.h's.
 *
 * Refusals, each by name and before any GPU call: a NULL block; NULL indices; topk == 0; reserved != 0; indexRowStride < topk; a
 * misaligned indices; and everything mfa_attention_mla_prefill_launch refuses for the same params, in its words.
 *
 * Kernels: attn_mla16px1_d576_<bf16|f16> (64 KiB of LDS, two workgroups a compute unit).
 *
 * Deliberately not here: e4m3 latent caches under prefill lists; pieces of slots with a combine pass (few rows under a long list leave
 * compute units idle); ragged (packed-axis) rows.  (A chunk's lists, any number of rows in one call, are mfa_mla_index_prefill.h's.)
 */
#ifndef MFA_MLA_PREFILL_SPARSE_H
#define MFA_MLA_PREFILL_SPARSE_H

#include "mfa_mla_prefill.h"
#include "mfa_mla_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the block is looked at first, then the params */
mfa_status mfa_attention_mla_prefill_sparse_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                   const mfa_mla_sparse *sparse, void *stream);

/* what a launch with these parameters runs, as text: the kernel, the grid with its factors (groups x rows x sequences), topk and the
 * layout; nothing is launched.  A NULL `out` or a zero capacity is refused after the block and ahead of the params */
mfa_status mfa_attention_mla_prefill_sparse_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_sparse *sparse, char *out,
                                                        size_t capacity);

/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_attention_mla_prefill_sparse_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                 const mfa_mla_sparse *sparse, void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_PREFILL_SPARSE_H */
