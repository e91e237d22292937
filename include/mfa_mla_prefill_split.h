/*
 * mfa_mla_prefill_split.h -- C ABI of KEY PIECES for multi-head latent attention PREFILL over the compressed KV cache: the launch of
 * mfa_mla_prefill.h cut along the KEYS, as decode (mfa_decode.h), prefill over the plain cache (mfa_split.h) and MLA decode (mfa_mla.h)
 * are.  A launch of few row blocks over a long cache -- a chunk of a chunked prefill, the rows behind a reused prefix of one long
 * conversation -- is a handful of workgroups that each walk the whole cache alone (64 rows x 16 heads: 16 workgroups on 256 compute
 * units); cut into pieces, the same launch fills the chip.  The key pieces mfa_mla_prefill.h names as "deliberately not here" live
 * HERE: that header, its struct and its entries are unchanged and run what they ran.  The rules of mfa_mla_prefill.h hold word for
 * word: plain pointers and sizes, caller-owned device memory, status codes, validation before any GPU call, every refusal names the
 * requirement, asynchronous launches that copy nothing to the host and never synchronise (graph-capturable: a straight chain of two
 * kernels, no atomics, no host reads).
 *
 * Operands, layouts, the mask, the packing (p = row x heads + head, blocks of MFA_MLA_PREFILL_PACKED_ROWS = 64), queryLengths, the
 * poison rules and the refusals are mfa_mla_prefill.h's word for word; the params struct is mfa_mla_prefill_params, unchanged (168
 * bytes).  The split is mfa_key_split of mfa_split.h, reused as it is -- `workspace`, `workspaceBytes`, `pieces` (0 = the host's plan,
 * 1 = unsplit, 2 .. MFA_MLA_PREFILL_SPLIT_MAX_PIECES = as given, more is refused), `reserved` = 0 -- and is required: NULL is refused.
 *
 * When the launch is not cut.  A NULL workspace, or one piece, runs mfa_attention_mla_prefill_launch: the kernel
 * attn_mla16p_d576_<type> on its grid, the unsplit launch bit for bit.  The launch form then says so ("unsplit without a workspace:
 * the plan has N pieces").
 *
 * The pieces.  A block of 64 packed rows of a sequence walks the 32-key steps [0, end) of mfa_attention_mla_prefill_step_range.  Piece
 * i of P takes the steps [i end / P, (i + 1) end / P) (64-bit products): mfa_attention_mla_prefill_split_piece_range, the kernels' own
 * function.  Whether a step runs with the per-element mask stays a property of the step (below firstMasked: without).  Each block cuts
 * its OWN range, so the causal blocks near the top of a chunk and those near its end get equal shares.  A piece without a step
 * publishes (m, l) = (-FLT_MAX, 0) for the block's live rows and writes no O.  A block whose first row is at or past queryLengths[b]
 * returns at once and publishes nothing.
 *
 * The workspace.  The project's one formula with `rows` the capacity: pieces x batches x heads x rows x (512 + 2) x 4 bytes -- slabs
 * wsO[piece][batch][packed p][512] of un-normalised O and, behind them, wsML[piece][batch][packed p][2] = (m, l), all FP32.  16-byte
 * aligned.  Never assumed zeroed; nothing of it is read that the same launch did not write.  A short or a misaligned workspace is
 * MFA_ERR_INVALID_ARGUMENT in decode's words, naming mfa_attention_mla_prefill_split_workspace_size.
 *
 * The combine kernel.  One wave per packed row of the capacity, lane s holding (m_s, l_s) of piece s.  Rows at or past queryLengths[b]
 * return before reading anything and are not written.  The weights are exp2(m_s - m*); a piece's O is read only where its l > 0.  A
 * live row without a visible key in any piece gets O = 0 and L = -FLT_MAX, the unsplit launch's answer.  The arithmetic and its order
 * are MLA decode's combine; the 16-bit / FP32 stores of O and L are the unsplit launch's.
 *
 * The plan (pieces = 0) sees batches, heads, rows and column only -- the lengths live on the device:
 *       blocks = batches x ceil(rows x heads / 64), steps = ceil(column / 32)
 *       pieces = min(TARGET / blocks, steps / MIN_STEPS, MAX_PIECES), below 2: 1
 * MFA_MLA_PREFILL_SPLIT_TARGET = 256: mfa_split.h's rule, 256 compute units x the workgroups per compute unit the kernel's LDS allows --
 * 96 KiB allow one.  MFA_MLA_PREFILL_SPLIT_MIN_STEPS = 16, argued from bytes as mfa_split.h argues its 8 tiles: a block-piece's slab is
 * 64 x 514 x 4 B = 132 KB, written once and read once; a step's cache rows are 32 x 576 x 2 B = 37 KB; sixteen steps keep the
 * workspace traffic at 0.45 of the cache traffic, the ratio MLA decode's 4 tiles give its 32-row slab.  What was measured is with the
 * constants below.
 *
 * Out of scope here: e4m3 latent caches under prefill; ragged (packed-axis) rows; lists of key positions; a window, sinks, a soft cap or
 * trees; the split as the default of the torch binding's flash_mla_prefill; moving decode onto blocks of 64 rows.
 * Kernels: attn_mla16pk_d576_<bf16|f16> (a piece), attn_mla16p_d576_<bf16|f16>_combine.
 */
#ifndef MFA_MLA_PREFILL_SPLIT_H
#define MFA_MLA_PREFILL_SPLIT_H

#include "mfa_mla_prefill.h"
#include "mfa_split.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_MLA_PREFILL_SPLIT_MAX_PIECES 64u   /* a lane of the combine kernel's wave per piece */
#define MFA_MLA_PREFILL_SPLIT_TARGET 256u      /* workgroups the plan aims at.  Measured (MI355X, bf16, B = 1, H = 16; the pieces
                                                  a target of 256 / of 512 gives): 64 rows over 32768 keys 222.1 us at 16 pieces / 241.7 at 32;
                                                  512 rows over 4096 keys 240.8 at 2 / 254.3 at 4; over 32768 keys 1478 at 2 / 1519 at 4 */
#define MFA_MLA_PREFILL_SPLIT_MIN_STEPS 16u    /* 32-key steps a planned piece keeps.  Measured (the same sweep): the constant binds on one of
                                                  the four rows, 64 rows over 4096 keys -- 119.2 us at 32 steps a piece (4 pieces), 72.9 at 16
                                                  (8), 54.2 at 8 (16), beyond the spread of 1 - 2 us; on the other three the target decides and
                                                  8 / 16 / 32 choose the same pieces.  One row of four is not most of them: 16 stays, and 8 is the
                                                  first thing to try where chunks of 64 rows behind prefixes of a few thousand keys matter */

/* the entries of mfa_mla_prefill.h with `split` after `params`.  `split` is required */
mfa_status mfa_attention_mla_prefill_split_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                  const mfa_key_split *split, void *stream);

/* what a launch with these parameters runs, as text: the kernels' names and their grids; nothing is launched */
mfa_status mfa_attention_mla_prefill_split_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split, char *out,
                                                       size_t capacity);

/* `iterations` back-to-back launches (both kernels of a cut launch) between two HIP events on `stream` */
mfa_status mfa_attention_mla_prefill_split_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                const mfa_key_split *split, void *stream, int warmup, int iterations, float *milliseconds);

/* *bytes: the workspace the launch needs to run in the pieces `split->pieces` asks for (0: the plan's), 0 when that is one piece;
 * *pieces (may be NULL): that piece count.  The workspace `split` may already name is not looked at */
mfa_status mfa_attention_mla_prefill_split_workspace_size(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                          uint64_t *bytes, uint32_t *pieces);

/* the kernels' own piece function, on the host: piece `piece` of `pieces` of a block whose walk is the steps [0, end) takes
 * [*beginStep, *endStep) = [piece x end / pieces, (piece + 1) x end / pieces) */
mfa_status mfa_attention_mla_prefill_split_piece_range(uint32_t end, uint32_t pieces, uint32_t piece, uint32_t *beginStep,
                                                       uint32_t *endStep);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_PREFILL_SPLIT_H */
