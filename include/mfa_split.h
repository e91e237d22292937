/*
 * mfa_split.h -- C ABI of KEY SPLITS for prefill over a KV cache: the prefill launches of mfa_prefill.h / mfa_window.h / mfa_sink.h /
 * mfa_tree.h (padded rows, any window and sinks, with or without a speculation tree) cut along the KEYS, as decode's launches are
 * (mfa_decode.h).  A launch of few row blocks -- one sequence, a speculation tree of 16 nodes, a short chunk of a chunked prefill --
 * is a handful of workgroups that each walk the whole cache alone; cut into pieces, the same launch fills the chip.  An extension of
 * mfa_tree.h, whose rules hold here word for word: plain pointers and sizes, caller-owned device memory, status codes, validation
 * before any GPU call, every refusal names the requirement, asynchronous launches that copy nothing to the host and never synchronise
 * (graph-capturable: a straight chain of two kernels, no atomics).  Existing structs and entries are unchanged and run what they
 * ran; the split is one small block, mfa_key_split, after `tree` in the entries below.
 *
 * The block.  `pieces`: 0 = the host's plan, 1 = the unsplit launch, 2 .. MFA_PREFILL_SPLIT_MAX_PIECES = as given; more is refused.
 * `workspace` (device, 16-byte aligned, `workspaceBytes` bytes): NULL runs the unsplit kernel of the other headers and is correct
 * (decode's rule).  A workspace smaller than the launch needs, or a misaligned one, is MFA_ERR_INVALID_ARGUMENT in decode's words.
 * The workspace is never assumed zeroed and nothing of it is read that the same launch did not write.
 *
 * The workspace.  pieces x batches x heads x rows x (D + 2) x 4 bytes (`rows` the capacity) -- the project's one formula: slabs
 * wsO[piece][batch][head][row][D] of un-normalised O and, behind them, wsML[piece][batch][head][row][2] = (m, l), all FP32.
 *
 * The pieces.  A row block walks the tile LIST [0, sinkEnd) ++ [begin, end) of its own five indices
 * (mfa_attention_prefill_sink_tile_range; with a tree mfa_attention_prefill_tree_tile_range, the same for every row block).  Piece i of
 * P takes the positions [i W / P, (i + 1) W / P) of that list of W tiles: mfa_attention_prefill_split_piece_range, the kernels' own
 * function.  Whether a tile runs with the per-element mask stays a property of the tile.  A piece without a tile publishes
 * (m, l) = (-FLT_MAX, 0) for its live rows; rows at or past queryLengths[b] publish nothing and are not merged or written.
 * The combine kernel merges a row's pieces by the weights exp2(m_s - m*), reads a piece's O only where its l > 0, and is where the
 * sink logit joins the denominator and the value scale multiplies O -- each exactly once per row, whichever pieces are empty.
 * A live row without a visible key in any piece gets O = 0 and L = -FLT_MAX, or the sink logit: the unsplit launch's answer.
 *
 * The plan (pieces = 0) sees batches, K/V heads, row blocks, column, rows, the window and the sink tokens only -- the lengths live on
 * the device: with `blocks` the unsplit grid and `tiles` decode's tile count of (column, rows, window, sink tokens),
 *       pieces = min(target / blocks, tiles / MFA_PREFILL_SPLIT_MIN_TILES, MFA_PREFILL_SPLIT_MAX_PIECES), below 2: 1
 * target = MFA_PREFILL_SPLIT_COMPUTE_UNITS x the workgroups per compute unit the kernel's LDS allows (2 at D <= 128, 1 at D = 256).
 *
 * Not here: ragged launches (mfa_ragged.h) and a soft cap (mfa_softcap.h) have no split kernel and no entry.
 * Kernels: attn_prefill16sk_*[_e4m3] (the sink body: plain, window and sink launches), attn_prefill16tk_*[_e4m3] (the tree body),
 * attn_prefill16_combine_d<D>_<type>.
 */
#ifndef MFA_SPLIT_H
#define MFA_SPLIT_H

#include "mfa_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_PREFILL_SPLIT_MAX_PIECES 64u    /* a lane of the combine kernel's wave per piece */
#define MFA_PREFILL_SPLIT_MIN_TILES 8u      /* tiles a planned piece keeps.  Argued from bytes: at D = 128 a piece's slab is 128 rows x (D + 2) x
                                               4 B = 66 KB, written once and read once -- the traffic of four 32 KB K / V tiles; eight tiles keep
                                               the workspace at or below half the cache traffic.  Measured (MI355X, B = 1, 32k keys, D = 128,
                                               DESIGN.md 4.20): a 16-node tree runs 52.8 us at 16 tiles a piece and 56.0 us at 8, the plan's choice */
#define MFA_PREFILL_SPLIT_COMPUTE_UNITS 256u /* the plan aims at this many times the workgroups per compute unit.  Measured (the same sweep): a
                                               128-row chunk is fastest at 512 workgroups (193 us; 205 at 1024, 312 at 256) */

typedef struct mfa_key_split {
  void *workspace;         /* device, 16-byte aligned; NULL: the unsplit launch */
  uint64_t workspaceBytes;
  uint32_t pieces;         /* 0 = planned, 1 = unsplit, 2 .. 64 = as given */
  uint32_t reserved;       /* 0 */
} mfa_key_split;

/* zeroes the block: no workspace, planned pieces */
void mfa_key_split_init(mfa_key_split *split);

/* sizeof(mfa_key_split), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity` are
 * written): what a binding's mirror of the struct is checked against */
size_t mfa_key_split_size(void);
mfa_status mfa_key_split_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* the prefill entries of mfa_tree.h with `split` after `tree` (`window` 0: none; `sinks` NULL: none; `tree` NULL: the causal rule of
 * mfa_prefill.h).  `split` is required */
mfa_status mfa_attention_prefill_split_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                              const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                              const mfa_attention_tree *tree, const mfa_key_split *split, void *stream);
mfa_status mfa_attention_prefill_split_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                   const mfa_attention_tree *tree, const mfa_key_split *split, char *out, size_t capacity);
mfa_status mfa_attention_prefill_split_time(const void *q, const void *k, const void *v, void *o, float *l,
                                            const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                            const mfa_attention_tree *tree, const mfa_key_split *split, void *stream, int warmup,
                                            int iterations, float *milliseconds);

/* *bytes: the workspace the launch needs to run in the pieces `split->pieces` asks for (0: the plan's), 0 when that is one piece;
 * *pieces (may be NULL): that piece count.  The workspace `split` may already name is not looked at */
mfa_status mfa_attention_prefill_split_workspace_size(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                      const mfa_attention_tree *tree, const mfa_key_split *split, uint64_t *bytes,
                                                      uint32_t *pieces);

/* the kernels' own piece function, on the host.  For a row block whose walked list is the tiles [0, sinkEnd) ++ [beginTile, endTile)
 * (sinkEnd <= beginTile <= endTile: three of the block's five indices), piece `piece` of `pieces` walks the tiles
 * [begin[0], end[0]) inside the sink tiles and then [begin[1], end[1]) inside [beginTile, endTile): the positions
 * [piece W / pieces, (piece + 1) W / pieces) of the list of W = sinkEnd + endTile - beginTile tiles. */
mfa_status mfa_attention_prefill_split_piece_range(uint32_t beginTile, uint32_t endTile, uint32_t sinkEnd, uint32_t pieces, uint32_t piece,
                                                   uint32_t begin[2], uint32_t end[2]);

#ifdef __cplusplus
}
#endif
#endif /* MFA_SPLIT_H */
