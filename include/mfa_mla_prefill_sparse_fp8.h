/*
 * mfa_mla_prefill_sparse_fp8.h -- C ABI of SPARSE multi-head latent attention PREFILL over an E4M3 latent cache: the rule of
 * mfa_mla_prefill_sparse.h (a block of query rows of any length, each over its own list of key positions, shared by all heads) over the
 * cache format of mfa_mla_cache.h (576 bytes a key, one FP32 scale) -- the prompt chunk of DeepSeek-V3.2 as it is served.  What
 * mfa_mla_prefill_sparse.h names "deliberately not here: e4m3 latent caches under prefill lists" is BUILT HERE, as entries of their own;
 * the headers this one includes are unchanged, no struct is added and mfa_abi_version() stays 6.  There is no workspace.
 *
 * The entries take the UNCHANGED mfa_mla_prefill_params (precision = the 16-bit type of Q; the KV strides count BYTES and are multiples
 * of 16; the cache pointer is 16-byte aligned), then mfa_mla_sparse (mfa_mla_sparse.h), then mfa_mla_quant (mfa_mla_cache.h).  A stored
 * byte b stands for kvScale[0] x e4m3(b); kvScale NULL = 1.0; the host reads neither the scale, the lists nor a length: one capture in
 * a graph serves changed lists and lengths.
 *
 * The rule is mfa_mla_prefill_sparse.h's, restated for bytes:
 * What an entry is.  indices[b][r][j] is a key POSITION c of sequence b, a logical position; a paged launch translates it through the
 * block table as the dense launch does.
 * When a slot is visible.  With n = min(cacheLengths[b], column) and qn = min(queryLengths[b], rows), slot j of row r < qn is visible
 * iff 0 <= c < n and, with `causal`, c <= r + max(n - qn, 0).
 * Holes.  Any other value is a hole, anywhere in the list: -1, entries below -1, a position at or past n, a position past the causal
 * frontier, and the slots of a last partial step of 32.  Its score is replaced, never computed from; its 576 bytes are NEVER LOADED (the
 * row enters the step as zero bytes); its block-table entry is never read.  Nothing past slot topk - 1 of a list is read.
 * What is never read.  A key that no list of the launch names is never loaded either: such rows, pages and table entries may hold
 * anything, the NaN bytes 0x7f / 0xff included.  Rows at or past queryLengths[b] are neither read (Q, their lists) nor written (O, L).
 * Only kvScale[0] is read.
 * Repeated positions.  A position that appears twice in a list COUNTS TWICE.  Callers pass distinct positions.
 * Empty rows.  A row r < qn with no visible slot gets O = 0 and L = -FLT_MAX.
 *
 * Packing is mfa_mla_prefill_sparse.h's: a workgroup serves 32 HEADS of ONE (sequence, row), head = 32 group + q; the grid is
 * batches x rows x groups, group fastest.  The scale folds as in every launch over the e4m3 cache: the score scale is
 * fl(fl(scale x log2 e) x kvScale), the last multiplication is by fl(fl(1 / l) x kvScale).
 *
 * Two identities, bit for bit in O and L.  For every row the arithmetic is that of mfa_mla_sparse_fp8.h's unsplit kernel: a launch of
 * up to 32 full rows (queryLengths NULL or = rows) equals mfa_attention_mla_sparse_decode_fp8_launch at one piece on the same inputs,
 * and a row's result does not depend on how a prompt is cut into launches.  With the list 0 .. column - 1 it is
 * mfa_attention_mla_prefill_fp8_launch's.
 *
 * Order of the refusals, each by name and before any GPU call:
 *   1. the sparse block, in mfa_mla_sparse.h's words: a NULL block; NULL indices; topk == 0; reserved != 0; indexRowStride < topk; a
 *      misaligned indices;
 *   2. the quant block, in mfa_mla_prefill_fp8.h's words: a NULL block; a cachePrecision other than MFA_KV_E4M3; reserved != 0;
 *   3. launch_form's NULL `out` or zero capacity;
 *   4. everything mfa_attention_mla_prefill_fp8_launch refuses for the same params, in its words;
 *   5. the grid's size: groups x rows x batches must fit 2^31 - 1 workgroups;
 *   6. Q, KV or O NULL or not 16-byte aligned, L or kvScale not 4-byte aligned.
 *
 * Kernels: attn_mla8px1_d576_<bf16|f16> (64 KiB of LDS: four 8 KiB V images and two 16 KiB exchange buffers; two workgroups a compute
 * unit).
 *
 * Deliberately not here: pieces of slots with a combine pass (few rows under a long list leave compute units idle); a workgroup of 64
 * heads; e5m2; per-token or per-128-column scales; a fused index + attend launch; ragged (packed-axis) rows.
 */
#ifndef MFA_MLA_PREFILL_SPARSE_FP8_H
#define MFA_MLA_PREFILL_SPARSE_FP8_H

#include "mfa_mla_cache.h"
#include "mfa_mla_prefill.h"
#include "mfa_mla_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the three entries of mfa_mla_prefill_sparse.h for an E4M3 latent cache; the sparse block is looked at first, then the quant block,
 * then the params */
mfa_status mfa_attention_mla_prefill_sparse_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                       const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream);

/* what a launch with these parameters runs, as text: the kernel, the grid with its factors (groups x rows x sequences), topk and the
 * layout; nothing is launched.  A NULL `out` or a zero capacity is refused after the blocks and ahead of the params */
mfa_status mfa_attention_mla_prefill_sparse_fp8_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_sparse *sparse,
                                                            const mfa_mla_quant *quant, char *out, size_t capacity);

/* `iterations` back-to-back launches between two HIP events on `stream` */
mfa_status mfa_attention_mla_prefill_sparse_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                     const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream, int warmup,
                                                     int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_PREFILL_SPARSE_FP8_H */
