/*
 * mfa_mla_sparse_fp8.h -- C ABI of SPARSE multi-head latent attention decode over an E4M3 latent cache: the rule of mfa_mla_sparse.h
 * (a per-row list of key positions, shared by all heads) over the cache format of mfa_mla_cache.h (576 bytes a key, one FP32 scale) --
 * the decode step of DeepSeek-V3.2 as it is served: an indexer picks 2048 keys per query token out of an FP8 latent cache.  What
 * mfa_mla_sparse.h names "deliberately not here: e4m3 latent caches under a list" is BUILT HERE, as entries of their own; the three
 * headers this one includes are unchanged, no struct is added and mfa_abi_version() stays 6.
 *
 * The entries take the UNCHANGED mfa_mla_decode_params (precision = the 16-bit type of Q; the KV strides in elements = bytes, multiples
 * of 16), then mfa_mla_sparse (mfa_mla_sparse.h), then mfa_mla_quant (mfa_mla_cache.h).  A stored byte b stands for
 * kvScale[0] x e4m3(b); kvScale NULL = 1.0; the host never reads the scale or the lists.
 *
 * Order of the refusals, each by name and before any GPU call:
 *   1. the sparse block, in mfa_mla_sparse.h's words: a NULL block; NULL indices; topk == 0; reserved != 0; indexRowStride < topk; a
 *      misaligned indices;
 *   2. the quant block, in mfa_mla_cache.h's words: a NULL block; a cachePrecision other than MFA_KV_E4M3;
 *   3. everything the dense e4m3 launch (mfa_attention_mla_decode_fp8_*) refuses for the same params, in its words;
 *   4. the grid's size (groups x rows x batches x pieces) and the workspace, in decode's words, naming
 *      mfa_attention_mla_sparse_decode_fp8_workspace_size.
 *
 * The rule is mfa_mla_sparse.h's, whatever that header says, restated for bytes:
 * What an entry is.  indices[b][r][j] is a key POSITION c of sequence b, a logical position; a paged launch translates it through the
 * block table as the dense launch does.
 * When a slot is visible.  Slot j is visible to row r iff 0 <= c < min(cacheLengths[b], column) and, with `causal`,
 * c <= r + max(cacheLengths[b] - R, 0).
 * Holes.  Any other value is a hole, anywhere in the list: -1, a position at or past the length, a position past the causal frontier.
 * Its score is replaced, never computed from; its 576 bytes are NEVER LOADED (the row enters the step as zero bytes); its block-table
 * entry is never read.
 * What is never loaded.  A key that no list of the launch names is never loaded either: such rows, pages and table entries may hold
 * anything, the NaN bytes 0x7f / 0xff included.
 * Repeated positions.  A position that appears twice in a list COUNTS TWICE.  Callers pass distinct positions.
 * Order.  The order of a list is free; the result depends on it only through rounding.
 * Empty rows.  A row with no visible slot gets O = 0 and L = -FLT_MAX.
 *
 * Packing, pieces and workspace are mfa_mla_sparse.h's: a workgroup serves 32 HEADS of ONE (sequence, row) and one piece of the list's
 * SLOTS; the grid is batches x rows x groups x pieces, pieces fastest, then the group; the plan is choose_pieces(batches x rows x
 * groups, the 64-slot tiles of topk, MFA_DECODE_WORKGROUP_TARGET, 4 tiles, 64 pieces); piece s takes the slots
 * mfa_attention_decode_piece_range(topk, pieces, s).  The workspace size and the pieces equal
 * mfa_attention_mla_sparse_decode_workspace_size's for the same params; a NULL workspace runs unsplit and is correct.
 * Over the identity list (indices[b][r][j] = j, topk = column) and unsplit, O and L equal mfa_attention_mla_decode_fp8_launch's on the
 * same inputs bit for bit.
 *
 * Kernels: attn_mla8x_d576_<bf16|f16> (unsplit), attn_mla8x_d576_<type>_k (a piece of the slots), attn_mla8x_d576_<type>_combine (the
 * combine body of the dense launch, instantiated beside them).
 *
 * Deliberately not here: the 656-byte layout (a 16-bit rotary part) and per-token or per-128-column scales; physical-slot indices;
 * rows > 32; sharing one list between the rows of a sequence (each row has its own, and its own walk of the cache); more than 32
 * packed rows per workgroup.
 */
#ifndef MFA_MLA_SPARSE_FP8_H
#define MFA_MLA_SPARSE_FP8_H

#include "mfa_mla_cache.h"
#include "mfa_mla_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the four entries of mfa_mla_sparse.h for an E4M3 latent cache; the sparse block is looked at first, then the quant block.  *bytes and
 * *pieces (may be NULL) equal mfa_attention_mla_sparse_decode_workspace_size's */
mfa_status mfa_attention_mla_sparse_decode_fp8_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse,
                                                              const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces);
mfa_status mfa_attention_mla_sparse_decode_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                      const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream);
/* the kernel, the grid with its factors (groups x rows x sequences [x pieces]), topk, the layout and the combine kernel */
mfa_status mfa_attention_mla_sparse_decode_fp8_launch_form(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse,
                                                           const mfa_mla_quant *quant, char *out, size_t capacity);
mfa_status mfa_attention_mla_sparse_decode_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                    const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream, int warmup,
                                                    int iterations, float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* MFA_MLA_SPARSE_FP8_H */
