/*
 * mfa_mla_index_prefill.h -- C ABI of the PREFILL INDEXER: the launches of mfa_mla_index.h for a prompt chunk of ANY number of rows, the
 * producer of the lists mfa_mla_prefill_sparse.h consumes.  The same three stages -- index logits, top-k selection, their chain -- over
 * the UNCHANGED mfa_mla_index_params, read without the 32-row limit, and beside it one argument, as mfa_mla_prefill_sparse.h takes its
 * second block beside an unchanged first one:
 *
 *   queryLengths  device, uint32, [batches]; NULL = `rows` for every sequence.  The host never reads it.
 *
 * Everything else of the block -- QI, W, KI, logits, indices, their layouts, strides and alignments, paged caches, precision, Di = 128,
 * indexHeads 1 .. 64 -- means what it means in mfa_mla_index.h.  No existing struct or entry changes; mfa_mla_index.h's entries keep
 * their limit.  A launch copies nothing to the host and never synchronises: one capture in a graph serves changed lengths.
 *
 * Visibility is prefill's rule, exactly what mfa_mla_prefill_sparse.h applies to the lists it is handed.  With
 * n = min(cacheLengths[b], column) and qn = min(queryLengths[b], rows), row r < qn sees the PREFIX [0, v): v = n without `causal`,
 * v = min(n, r + max(n - qn, 0) + 1) with it.  (At queryLengths = NULL and rows <= 32 this is mfa_mla_index.h's rule.)
 *
 * mfa_mla_index_prefill_logits_launch.  For every row r < qn and every position c < v, mfa_mla_index.h's logit, by the same chain of
 * FP32 operations.  NOTHING ELSE IS WRITTEN: not positions at or past v, not rows at or past qn.  NEVER LOADED: keys at or past n, the
 * rest of a last page, pages the table does not name, table entries past the last page, and QI and W of rows at or past qn.
 * Work split -- the opposite of the decode indexer's: a workgroup is four waves that serve ONE sequence, one tile of
 * MFA_MLA_INDEX_PREFILL_TILE = 256 keys and a SPAN of rows.  A wave loads its 64 keys once and keeps them in registers; the rows stream
 * through a ring of two images in LDS, each row's queries copied once per workgroup in the matrix instruction's fragment order.  Grid:
 * tiles x spans x batches, tile fastest.  The host cuts the rows into spans of a multiple of MFA_MLA_INDEX_PREFILL_MIN_SPAN = 32 rows,
 * as many as bring the grid to 512 workgroups, and of at most MFA_MLA_INDEX_PREFILL_MAX_SPAN = 256 rows.  With `causal` a workgroup
 * starts at the first row whose prefix reaches its tile; a tile at or past n returns at once.
 *
 * mfa_mla_index_prefill_select_launch.  Rows r < qn get mfa_mla_index.h's list of logits[b][r][0 .. v): membership by "larger FP32 order
 * key first, lower position first", written in ascending position, then -1.  Rows at or past qn get topk slots of -1 and read no logit
 * (the sparse prefill never reads those lists; writing them keeps the result a pure function of the inputs).  One workgroup per
 * (sequence, row).
 *
 * mfa_mla_index_prefill_topk_launch.  A chunk's logits are batches x rows x column x 4 bytes -- 512 MiB per sequence at 4096 rows of
 * 32768 keys -- so the chain runs PASSES of rows, logits then select per pass, all enqueued on the caller's stream.  The workspace holds
 * [batches][pass rows][column rounded up to 4] floats; rows per pass = what workspaceBytes holds, rounded down to whole spans (all rows
 * if they fit).  A NULL workspace, one that cannot hold one span per sequence and a misaligned one are refused by name.
 * mfa_mla_index_prefill_workspace_size returns the smaller of the whole chunk and MFA_MLA_INDEX_PREFILL_WORKSPACE_CAP = 256 MiB in
 * whole spans (one span per sequence where even that exceeds the cap).  A row's result does not depend on the pass it falls in: the
 * chain equals the select launch applied to the logits launch, bit for bit, for every admissible workspace.
 *
 * Refusals: mfa_mla_index.h's, in its order and words and before any GPU call, without "at most 32 rows"; the grid factors
 * (tiles x spans x batches; rows x batches) must fit 2^31 - 1.
 *
 * launch_form prints the kernels with their grids' factors -- tiles of 256 keys, spans and their rows, sequences -- and, for the chain,
 * the passes and their rows; the grids are the first pass's.
 *
 * Kernels: attn_mlaip_d128_<bf16|f16> (logits; 32.5 KiB of LDS, two workgroups a compute unit), attn_mlaip_select.
 *
 * Deliberately not here: a fused logits + select that never materialises the logits; e4m3 index caches and per-key scales; an FP8
 * matrix-instruction path; ragged (packed-axis) rows; an eight-wave tile of 512 keys; cutting one row's selection across several
 * workgroups.
 */
#ifndef MFA_MLA_INDEX_PREFILL_H
#define MFA_MLA_INDEX_PREFILL_H

#include "mfa_mla_index.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_MLA_INDEX_PREFILL_TILE 256                      /* keys of a logits workgroup */
#define MFA_MLA_INDEX_PREFILL_MIN_SPAN 32                   /* rows: a span is a multiple of it */
#define MFA_MLA_INDEX_PREFILL_MAX_SPAN 256                  /* rows: ... and never longer */
#define MFA_MLA_INDEX_PREFILL_WORKSPACE_CAP (256ull << 20)  /* bytes: what workspace_size recommends at most */

/* *bytes: the workspace mfa_mla_index_prefill_topk_launch should be given (see above).  The workspace the params may already carry is
 * not looked at. */
mfa_status mfa_mla_index_prefill_workspace_size(const mfa_mla_index_params *params, const uint32_t *queryLengths, uint64_t *bytes);

mfa_status mfa_mla_index_prefill_logits_launch(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                               const uint32_t *queryLengths, void *stream);
/* what a launch with these parameters runs, as text; nothing is launched */
mfa_status mfa_mla_index_prefill_logits_launch_form(const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity);
/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_mla_index_prefill_logits_time(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                             const uint32_t *queryLengths, void *stream, int warmup, int iterations, float *milliseconds);

mfa_status mfa_mla_index_prefill_select_launch(const float *logits, int32_t *indices, const mfa_mla_index_params *params,
                                               const uint32_t *queryLengths, void *stream);
mfa_status mfa_mla_index_prefill_select_launch_form(const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity);
mfa_status mfa_mla_index_prefill_select_time(const float *logits, int32_t *indices, const mfa_mla_index_params *params, const uint32_t *queryLengths,
                                             void *stream, int warmup, int iterations, float *milliseconds);

mfa_status mfa_mla_index_prefill_topk_launch(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                             const uint32_t *queryLengths, void *stream);
mfa_status mfa_mla_index_prefill_topk_launch_form(const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity);
mfa_status mfa_mla_index_prefill_topk_time(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                           const uint32_t *queryLengths, void *stream, int warmup, int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_INDEX_PREFILL_H */
