/*
 * mfa_ragged.h -- C ABI of RAGGED BATCHES over a KV cache: the prefill launch and the cache append for the batch shape a
 * continuous-batching engine hands over -- sequences with one new token beside sequences with a prompt chunk of thousands, their
 * rows PACKED along one axis (q [totalRows][heads][D], kNew / vNew [totalRows][K/V heads][D]) with a device array of row starts
 * (`cu_seqlens_q` / `query_start_loc`).  No copy into a padded layout, no workgroup for a row block that does not exist, one append
 * launch for the whole batch.  An extension of mfa_sink.h, whose rules hold here word for word: plain pointers and sizes,
 * caller-owned device memory, status codes, validation before any GPU call, every refusal names the requirement, asynchronous
 * launches that copy nothing to the host and never synchronise (graph-capturable).  No existing struct, entry, kernel, launch-form
 * text or workspace size changes; the packing is one small block, mfa_ragged_rows, after `sinks` in the entries below.
 *
 * The rule.  With T = totalRows, s_b = min(rowStarts[b], T) and e_b = min(rowStarts[b + 1], T):
 *   sequence b owns the packed rows [s_b, s_b + qn_b),  qn_b = min(max(e_b - s_b, 0), params->rows)   (no unsigned wrap-around);
 *   params->rows is the LARGEST row count of any sequence: a cap, not a capacity.
 *   Row r of sequence b, head h:   Q + h headStride[Q] + (s_b + r) leadingDimension[Q];   O likewise;   L + h lHeadStride + (s_b + r).
 * Everything else is mfa_prefill.h / mfa_window.h / mfa_sink.h with queryLengths[b] replaced by qn_b: the mask, n, lim, lo, sink
 * tokens and logits, rows without a visible key, what is never loaded, FP8 scales.  Packed rows at or past T are never read or
 * written, nor are the rows between s_b + qn_b and the next sequence's start.  Starts that DECREASE give an unspecified set of
 * computed rows (a sequence whose end lies below its start has qn = 0), but never an access outside the rows [0, T).
 *
 * Refusals, each MFA_ERR_INVALID_ARGUMENT naming the field: a NULL block, NULL rowStarts, totalRows = 0,
 * params->queryLengths != NULL (the starts give the counts), a non-zero batchStride of Q or O (kNew, vNew) or a non-zero
 * lBatchStride (the packed layout has no batch axis).  The stride and alignment rules of mfa_prefill.h / mfa_kvcache.h hold
 * unchanged.
 *
 * Prefill.  The entries take mfa_sink.h's signature plus `ragged` after `sinks`; sinks == NULL: none, window == 0: none.  They
 * always run the attn_prefill16r_* kernels: the sink kernels' body with the packed addressing, so one kernel serves plain, window
 * and sink launches, byte for byte what the padded launch of the same sequences computes.
 *   The grid is TIGHT: slots x K/V heads workgroups, slots = min(T / RB + batches, batches x ceil(rows / RB)) with RB = 128 / G and
 *   integer division -- an upper bound of sum_b ceil(qn_b / RB) for non-decreasing starts (ceil(x / RB) <= x / RB + 1 with integer
 *   division, and the sequences' rows are disjoint inside [0, T)).  Slot i serves row block i - sum_{j < b} ceil(qn_j / RB) of the
 *   sequence b in which it falls; a slot past the total returns at once (mfa_attention_prefill_ragged_block: the kernels' own
 *   function).  The order in which slots start is free and results do not depend on it.
 *
 * Append.  kNew, vNew packed the same way (batchStride 0, params->rows the cap); row r of sequence b goes to key
 * cacheLengths[b] - qn_b + r, under the drop rules of mfa_kvcache.h (a negative index, an index >= column, a page index past the
 * table).  One workgroup per packed row: kv_cache_append_ragged_*.
 */
#ifndef MFA_RAGGED_H
#define MFA_RAGGED_H

#include "mfa_sink.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfa_ragged_rows {
  const uint32_t *rowStarts;   /* device, [batches + 1], non-decreasing; the host never reads it */
  uint32_t totalRows;          /* T: packed rows of Q / O / L (or kNew / vNew); rows at or past T are never read or written */
  uint32_t reserved;           /* 0 */
} mfa_ragged_rows;

/* zeroes the block */
void mfa_ragged_rows_init(mfa_ragged_rows *ragged);

/* sizeof(mfa_ragged_rows), and offsetof of its fields in declaration order (`count` receives their number; at most `capacity` are
 * written): what a binding's mirror of the struct is checked against */
size_t mfa_ragged_rows_size(void);
mfa_status mfa_ragged_rows_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count);

/* the prefill entries of mfa_sink.h with `ragged` after `sinks` (`sinks` NULL: none; `window` 0: none) */
mfa_status mfa_attention_prefill_ragged_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                               const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                               const mfa_ragged_rows *ragged, void *stream);
mfa_status mfa_attention_prefill_ragged_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                    const mfa_ragged_rows *ragged, char *out, size_t capacity);
mfa_status mfa_attention_prefill_ragged_time(const void *q, const void *k, const void *v, void *o, float *l,
                                             const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                             const mfa_ragged_rows *ragged, void *stream, int warmup, int iterations,
                                             float *milliseconds);

/* the slots of a launch: min(totalRows / blockRows + batches, batches x ceil(rows / blockRows)) */
mfa_status mfa_attention_prefill_ragged_slots(uint32_t totalRows, uint32_t batches, uint32_t rows, uint32_t blockRows, uint64_t *slots);

/* the kernels' own slot function, on HOST arrays: rowStarts [batches + 1].  *sequence = the sequence slot `slot` serves and
 * *firstRow = the first row (of that sequence) of its row block, a multiple of blockRows; a slot at or past
 * sum_b ceil(qn_b / blockRows): *sequence = UINT32_MAX, *firstRow = 0. */
mfa_status mfa_attention_prefill_ragged_block(const uint32_t *rowStarts, uint32_t batches, uint32_t totalRows, uint32_t rows,
                                              uint32_t blockRows, uint32_t slot, uint32_t *sequence, uint32_t *firstRow);

/* mfa_kv_cache_append_launch for packed sources */
mfa_status mfa_kv_cache_append_ragged_launch(const void *kNew, const void *vNew, void *kCache, void *vCache,
                                             const mfa_kv_append_params *params, const mfa_ragged_rows *ragged, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MFA_RAGGED_H */
