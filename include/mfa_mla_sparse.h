/*
 * mfa_mla_sparse.h -- C ABI of SPARSE multi-head latent attention decode: the launch of mfa_mla.h over a per-row list of selected keys
 * instead of over every key below the length -- the decode step of DeepSeek-V3.2, whose indexer picks 2048 keys per query token,
 * shared by all heads, out of the same 576-wide latent cache.  mfa_mla.h's rule with one more operand: mfa_mla_decode_params is passed
 * unchanged (Q, the cache and its layouts, O, L, scale, cacheLengths, causal, rows <= 32, precision: all as there, a 16-bit cache), and
 * beside it goes mfa_mla_sparse, passed the way mfa_mla_quant is.  No existing struct or entry changes.
 *
 *   indices  [batches][rows][topk]  int32, device: the list of row r of sequence b starts at indices + b indexBatchStride +
 *            r indexRowStride and has `topk` slots; every head of that row attends to the same list.
 *
 * What an entry is.  indices[b][r][j] is a key POSITION c of sequence b: a logical position, not a physical slot of the cache.  A paged
 * launch translates it through the block table exactly as the dense launch does.
 * When a slot is visible.  Slot j is visible to row r iff 0 <= c < min(cacheLengths[b], column) and, with `causal`,
 * c <= r + max(cacheLengths[b] - R, 0).
 * Holes.  Any other value is a hole, anywhere in the list: -1, a position at or past the length, a position past the causal frontier.
 * Its score is replaced, never computed from; its cache row is NEVER LOADED; its block-table entry is never read.
 * What is never loaded.  A key that no list of the launch names is never loaded either: such rows, pages and table entries may hold
 * anything, NaN included.
 * Repeated positions.  A position that appears twice in a list COUNTS TWICE (two terms of the softmax).  Callers pass distinct positions.
 * Order.  The order of a list is free; the result depends on it only through rounding.
 * Empty rows.  A row with no visible slot gets O = 0 and L = -FLT_MAX.
 * Device reads.  The host never reads `indices`.
 * Pointer and stride.  `indices` is 4-byte aligned and indexRowStride >= topk; there is no other requirement on topk or the strides
 * (indexBatchStride 0 shares one set of lists between the sequences).  The kernels walk a list in steps of 32 slots; the slots of a
 * last partial step are holes, and nothing past slot topk - 1 of a list is read.
 *
 * Packing.  The rows packed into one workgroup must share one list, so a workgroup serves 32 HEADS of ONE (sequence, row) and one piece
 * of the list: groups = ceil(heads / 32), and the grid is batches x rows x groups x pieces, pieces fastest, then the group, so that the
 * groups of one (sequence, row) -- which read the same cache rows -- are neighbours.  Lanes of heads at or past `heads` repeat the last
 * head and store nothing.  rows <= 32 stays; heads >= 1 is free.
 *
 * Pieces are pieces of SLOTS.  `pieces`: 0 is the host's plan, 1 is unsplit, 2 .. 64 as given (mfa_split.h).  The plan is
 * choose_pieces(batches x rows x groups, the 64-slot tiles of topk, MFA_DECODE_WORKGROUP_TARGET, 4 tiles, 64 pieces).  Piece s takes the
 * slots mfa_attention_decode_piece_range(topk, pieces, s).  The workspace is the project's one formula, pieces x batches x heads x rows
 * x (Dv + 2) x 4 bytes, 16-byte aligned, never assumed zeroed; its slabs are indexed by the packed row head x rows + row, as mfa_mla.h's.
 * A NULL workspace runs unsplit and is correct; a short or misaligned one is refused in decode's words, naming
 * mfa_attention_mla_sparse_decode_workspace_size.
 *
 * Refusals, each by name and before any GPU call: a NULL block; NULL indices; topk == 0; reserved != 0; indexRowStride < topk; a
 * misaligned indices; and everything the dense launch refuses for the same params, in its words.
 *
 * Kernels: attn_mla16x_d576_<bf16|f16> (unsplit), attn_mla16x_d576_<type>_k (a piece of the slots), attn_mla16x_d576_<type>_combine
 * (the combine body of the dense launch, instantiated beside them).
 *
 * Deliberately not here: e4m3 latent caches under a list; physical-slot indices; per-row list lengths other than through -1; more than
 * 32 packed rows per workgroup; sharing one list between the rows of a sequence (each row has its own, and its own walk of the cache).
 */
#ifndef MFA_MLA_SPARSE_H
#define MFA_MLA_SPARSE_H

#include "mfa_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfa_mla_sparse {
  const int32_t *indices;     /* device, [batches][rows][topk] */
  uint32_t topk;              /* slots of a row's list, >= 1 */
  uint32_t reserved;          /* 0 */
  int64_t indexRowStride;     /* entries, >= topk */
  int64_t indexBatchStride;   /* entries */
} mfa_mla_sparse;

/* zeroes the block */
void mfa_mla_sparse_init(mfa_mla_sparse *sparse);

/* sizeof(mfa_mla_sparse), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity` are
 * written): what a binding's mirror of the struct is checked against */
size_t mfa_mla_sparse_size(void);
mfa_status mfa_mla_sparse_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* the four entries of mfa_mla.h for a launch over lists; the block is looked at first.  *bytes: pieces x batches x heads x rows x
 * (Dv + 2) x 4, 0 when the launch has one piece; *pieces (may be NULL): the plan for params->pieces = 0, else as given */
mfa_status mfa_attention_mla_sparse_decode_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse, uint64_t *bytes,
                                                          uint32_t *pieces);
mfa_status mfa_attention_mla_sparse_decode_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                  const mfa_mla_sparse *sparse, void *stream);
/* the kernel, the grid with its factors (groups x rows x sequences [x pieces]), topk, the layout and the combine kernel */
mfa_status mfa_attention_mla_sparse_decode_launch_form(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse, char *out,
                                                       size_t capacity);
mfa_status mfa_attention_mla_sparse_decode_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                const mfa_mla_sparse *sparse, void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_SPARSE_H */
