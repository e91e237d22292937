// mla_launch.h -- what the host sides of the six MLA attention launches share (attn_mla16.hip, attn_mla16_sparse.hip, attn_mla8_sparse.hip,
// attn_mla16_prefill.hip, attn_mla16_prefill_split.hip, attn_mla8_prefill.hip, attn_mla16_prefill_sparse.hip): the checks of the sparse,
// quant and split blocks; the checks mfa_mla_decode_params and mfa_mla_prefill_params are put to in the same words, and each launch's
// own on top of them (check_mla_decode_params, prepare_mla_prefill_args); the fields MlaArgs and MlaPrefillArgs have in common; the
// buffers of a launch; the cut along the keys (plan_mla_pieces) and the plan that runs it (MlaCutPlan); the sparse decode plan, which two
// units run over their own kernels; the bodies of the launch, time and workspace_size entries; and the launch forms that more than one
// entry speaks.  A unit keeps its kernels, its kernel table, what its plan alone knows -- the packing, the grid and its bound, the tiles a
// piece plan is chosen from -- and its entries, whose order of refusals is pinned by tests/golden/mla_refusals.json: where an entry
// judges a block, a NULL out-parameter and the params in an order of its own, those few lines stay with the entry.
// Internal, not part of the ABI.  Every check records its message (fail, mfa_internal.h) and returns the status.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla.h"
#include "../../include/mfa_mla_cache.h"
#include "../../include/mfa_mla_prefill.h"
#include "../../include/mfa_mla_prefill_split.h"
#include "../../include/mfa_mla_sparse.h"
#include "attn_mla16.h"
#include "attn_mla16_prefill.h"
#include "attn_mla16_sparse.h"
#include "cache_launch.h"
#include "mfa_internal.h"

namespace mfa {

// ---- the blocks

// mfa_mla_sparse, looked at before everything else: `otherwise` names the launch over every key and its entries
inline mfa_status check_mla_sparse(const mfa_mla_sparse *s, const char *otherwise) {
  if (!s)
    return fail(MFA_ERR_INVALID_ARGUMENT, std::string("null mfa_mla_sparse: the sparse entries require the block (mfa_mla_sparse_init; a launch over ") +
                                              otherwise + ")");
  if (!s->indices) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.indices is required (device array [batches][rows][topk] of int32 key positions)");
  if (s->topk == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.topk must be at least 1 (the slots of a row's list)");
  if (s->reserved != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.reserved must be 0, not " + std::to_string(s->reserved));
  if (s->indexRowStride < (int64_t)s->topk)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.indexRowStride must be at least topk = " + std::to_string(s->topk) + " entries, not " +
                                              std::to_string(s->indexRowStride));
  if ((uintptr_t)s->indices % 4 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.indices must be 4-byte aligned");
  return MFA_OK;
}
constexpr const char *kMlaDenseDecode = "every key below the length: the mfa_mla.h entries";
constexpr const char *kMlaDensePrefill = "every key below the frontier: the mfa_mla_prefill.h entries";

// mfa_mla_quant: required, and its cache is e4m3.  `entries`: the family that asks ("fp8", "fp8 prefill"); `header`: where a 16-bit
// latent cache is served; `reservedIsZero`: prefill refuses a non-zero `reserved`, decode never has
inline mfa_status check_mla_quant(const mfa_mla_quant *quant, const char *entries, const char *header, bool reservedIsZero) {
  if (!quant)
    return fail(MFA_ERR_INVALID_ARGUMENT, std::string("null mfa_mla_quant: the ") + entries + " entries require the block (mfa_mla_quant_init; a 16-bit latent "
                                              "cache: the " + header + " entries)");
  bool fp8 = false;
  const mfa_status st = check_cache_precision(quant->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3, not " + std::to_string(quant->cachePrecision) +
                                              " (a 16-bit latent cache: the " + header + " entries)");
  if (reservedIsZero && quant->reserved != 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_quant.reserved must be 0, not " + std::to_string(quant->reserved));
  return MFA_OK;
}
inline mfa_status check_mla_decode_quant(const mfa_mla_quant *quant) { return check_mla_quant(quant, "fp8", "mfa_mla.h", false); }

// mfa_key_split of the prefill entries that cut
inline mfa_status check_mla_prefill_split(const mfa_key_split *split) {
  if (!split)
    return fail(MFA_ERR_INVALID_ARGUMENT, "null mfa_key_split: the split entries require the block (mfa_key_split_init; the launch that is "
                                          "never cut: mfa_attention_mla_prefill_launch)");
  if (split->pieces > MFA_MLA_PREFILL_SPLIT_MAX_PIECES)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_key_split.pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64 (a lane of the combine kernel's "
                                          "wave per piece), not " + std::to_string(split->pieces));
  if (split->reserved != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_key_split.reserved must be 0");
  return MFA_OK;
}

// ---- the params

// What mfa_mla_decode_params and mfa_mla_prefill_params are refused for alike, in this order; `noun`: "decode" / "prefill".  `packing()`
// stands where each launch's own limits have always stood, between the sizes and cacheLengths: its rows, its pieces, its grid.
// `e4m3Rows`: decode over an e4m3 cache, whose KV strides count bytes, in multiples of 16, and whose precision is Q's.
template <typename Params, typename Packing>
mfa_status check_mla_params(const Params *p, const char *noun, bool e4m3Rows, Packing packing, uint32_t *pageShift) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, std::string("MLA ") + noun +
                                         (e4m3Rows ? " over an e4m3 latent cache takes a 16-bit Q (precision MFA_BF16 or MFA_FP16); an FP32 Q has no kernel"
                                                   : " reads 16-bit caches (MFA_BF16 or MFA_FP16); an FP32 cache has no kernel"));
  mfa_status st = check_precisions(p->precision, p->outputPrecision);
  if (st != MFA_OK) return st;
  if (p->headDimension != MFA_MLA_HEAD_DIMENSION || p->valueDimension != MFA_MLA_VALUE_DIMENSION)
    return fail(MFA_ERR_UNSUPPORTED, std::string("MLA ") + noun + " is compiled for (headDimension, valueDimension) = (576, 512), not (" +
                                         std::to_string(p->headDimension) + ", " + std::to_string(p->valueDimension) + ")");
  if (!(p->scale > 0.0f) || std::isinf(p->scale))   // (a NaN fails the comparison)
    return fail(MFA_ERR_INVALID_ARGUMENT, "scale is required: the model's softmax scale in natural units, finite and > 0 (there is no default), not " +
                                              std::to_string(p->scale));
  if ((st = check_sizes(p)) != MFA_OK) return st;
  if ((st = packing()) != MFA_OK) return st;
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  if ((st = check_paging(p->pageSize, p->blockTable, p->blockTableStride, p->column, pageShift)) != MFA_OK) return st;
  static const char *names[3] = {"Q", "KV", "O"};
  for (int i = 0; i < 3; ++i) {
    const int64_t outer = i == 1 && p->pageSize ? p->pageStride : p->batchStride[i];
    const bool bytes = i == 1 && e4m3Rows;   // rows of an e4m3 cache: an element is a byte
    st = check_operand_strides(names[i], i == 2 ? p->valueDimension : p->headDimension, p->leadingDimension[i], i == 1 ? 0 : p->headStride[i],
                               outer, i == 2 ? 4 : bytes ? 16 : 8,
                               bytes ? "(16-byte rows of an e4m3 cache)" : "(16-byte rows for Q and KV; whole 4-element stores for O)");
    if (st != MFA_OK) return st;
  }
  return MFA_OK;
}

// the fields MlaArgs and MlaPrefillArgs have in common, from checked params; the caller has zeroed its whole block, padding included
template <typename Args, typename Params>
void fill_mla_args(Args &a, const Params *p, uint32_t pageShift) {
  a.lengths = p->cacheLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride;   // (an e4m3 cache: bytes)
  a.ldo = p->leadingDimension[2]; a.hso = p->headStride[2]; a.bso = p->batchStride[2];
  a.lhs = p->lHeadStride; a.lbs = p->lBatchStride;
  a.R = p->rows; a.H = p->heads; a.batches = p->batches; a.column = p->column;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0; a.outF32 = p->outputPrecision == MFA_FP32;
  a.scale2 = p->scale * 1.44269504089f;   // fl(scale x log2 e)
}

// the buffers of a launch into its argument block; `kvScale`: the scale of an e4m3 cache (a 16-bit cache: null)
template <typename Args>
mfa_status bind_mla(Args &a, const float *kvScale, const void *q, const void *kv, void *o, float *l) {
  mfa_status st = check_buffers({q, kv, o}, "Q, KV and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st == MFA_OK) st = check_float_arrays({kvScale}, "kvScale");
  if (st != MFA_OK) return st;
  a.q = (const char *)q; a.kv = (const char *)kv; a.o = (char *)o; a.l = l;
  return MFA_OK;
}

// everything the dense decode launch refuses in mfa_mla_decode_params that needs neither a workspace nor a GPU, for the sparse launches
// over the same params too.  `e4m3Rows` as check_mla_params takes it.
inline mfa_status check_mla_decode_params(const mfa_mla_decode_params *p, bool e4m3Rows, uint32_t *pageShift) {
  return check_mla_params(p, "decode", e4m3Rows, [p]() {
    if (p->rows > MFA_MLA_PACKED_ROWS)
      return fail(MFA_ERR_UNSUPPORTED, "MLA decode takes at most 32 rows per sequence, not " + std::to_string(p->rows) +
                                           ": a longer block of query rows is a prefill, which is not served over the latent cache");
    if (p->pieces > MFA_DECODE_MAX_PIECES)
      return fail(MFA_ERR_INVALID_ARGUMENT, "pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. " + std::to_string(MFA_DECODE_MAX_PIECES) +
                                                ", not " + std::to_string(p->pieces));
    const uint64_t M = (uint64_t)p->heads * p->rows, groups = (M + MFA_MLA_PACKED_ROWS - 1) / MFA_MLA_PACKED_ROWS;
    if (M > 0x7FFFFFFFull || groups * p->batches * MFA_DECODE_MAX_PIECES > 0x7FFFFFFFull)
      return fail(MFA_ERR_INVALID_ARGUMENT, "groups x batches x pieces must fit a grid of 2^31 - 1 workgroups");
    return (mfa_status)MFA_OK;
  }, pageShift);
}

// every check of the unsplit 16-bit prefill launch that needs no GPU, in its words, for the cut, e4m3 and sparse launches over the same
// params too; on MFA_OK the fields of the zeroed `a` that come from the params are filled (buffer pointers null, no pieces)
inline mfa_status prepare_mla_prefill_args(const mfa_mla_prefill_params *p, MlaPrefillArgs &a) {
  uint32_t pageShift = 0;
  const mfa_status st = check_mla_params(p, "prefill", false, [p]() {
    const uint64_t M = (uint64_t)p->heads * p->rows, blocks = (M + MFA_MLA_PREFILL_PACKED_ROWS - 1) / MFA_MLA_PREFILL_PACKED_ROWS;
    if (M > 0x7FFFFFFFull || blocks * p->batches > 0x7FFFFFFFull)
      return fail(MFA_ERR_INVALID_ARGUMENT, "rows x heads, and blocks x batches, must fit a grid of 2^31 - 1 workgroups");
    return (mfa_status)MFA_OK;
  }, &pageShift);
  if (st != MFA_OK) return st;
  fill_mla_args(a, p, pageShift);
  a.qlengths = p->queryLengths;
  a.blocks = (uint32_t)(((uint64_t)p->heads * p->rows + MFA_MLA_PREFILL_PACKED_ROWS - 1) / MFA_MLA_PREFILL_PACKED_ROWS);
  return MFA_OK;
}

// ---- the cut along the keys

// a plan's kernels for one precision: [pieces > 1], and the combine kernel of its own translation unit (without relocatable device
// code a unit cannot launch another unit's kernel)
template <typename Args> struct MlaKernelSet {
  int precision;
  CacheKernel<Args> kernel[2];
  CacheKernel<Args> combine;
};
template <typename Set, size_t N> const Set *find_mla_set(const Set (&sets)[N], int precision) {
  for (const Set &s : sets)
    if (s.precision == precision) return &s;
  return nullptr;
}

// The piece count of a launch and its workspace: `asked` pieces, or (0) choose_pieces' from the workgroups the launch has unsplit and
// the `tiles` a sequence can walk; without a workspace the launch runs unsplit; a launch in more than one piece checks its workspace
// -- `sizeEntry` is the entry that says how many bytes -- and points the argument block's slabs into it.
template <typename Args>
mfa_status plan_mla_pieces(Args &a, uint32_t asked, uint64_t blocks, uint64_t tiles, uint64_t target, uint64_t minTiles, uint64_t maxPieces,
                           uint64_t rows, void *workspace, uint64_t workspaceBytes, const char *sizeEntry, uint32_t *planned, uint32_t *pieces) {
  *planned = asked ? asked : choose_pieces(blocks, tiles, target, minTiles, maxPieces);
  *pieces = workspace ? *planned : 1;   // no workspace: one kernel, unsplit
  if (*pieces == 1) return MFA_OK;
  const mfa_status st = check_split_workspace(workspace, workspaceBytes, split_workspace_bytes(*pieces, rows, MLA_DV), sizeEntry);
  if (st == MFA_OK) set_split_slabs(a, workspace, *pieces, rows, MLA_DV);
  return st;
}

// What the plans that can cut have in common.  A plan adds prepare(...), which fills everything here, and bind(q, kv, o, l).
template <typename Args, int LDS> struct MlaCutPlan {
  Args args;
  const MlaKernelSet<Args> *set;
  uint32_t pieces;      // as the launch runs: 1 without a workspace
  uint32_t planned;     // what the caller's `pieces` asks for: the host's plan, or as given
  uint32_t blocks;      // the workgroups of the unsplit launch
  uint64_t rows;        // batches x heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  const CacheKernel<Args> &kernel() const { return set->kernel[pieces > 1]; }
  const char *name() const { return kernel().name; }
  hipError_t run(hipStream_t stream) const { return run_pieces(kernel(), blocks, pieces, (uint32_t)LDS, set->combine, rows, stream, args); }
};

// the cut of a prefill launch whose `a` prepare_mla_prefill_args has filled: the split block's pieces or the plan over the 32-key steps
// of `column`, the block's workspace, and the grid of the cut launch
template <typename Plan>
mfa_status plan_mla_prefill_pieces(Plan *plan, MlaPrefillArgs &a, const mfa_mla_prefill_params *p, const mfa_key_split *split, const char *sizeEntry) {
  plan->blocks = a.blocks * a.batches;
  plan->rows = (uint64_t)p->batches * p->heads * p->rows;
  const uint64_t steps = ((uint64_t)p->column + MFA_MLA_PREFILL_KEY_STEP - 1) / MFA_MLA_PREFILL_KEY_STEP;
  const mfa_status st = plan_mla_pieces(a, split->pieces, plan->blocks, steps, MFA_MLA_PREFILL_SPLIT_TARGET, MFA_MLA_PREFILL_SPLIT_MIN_STEPS,
                                        MFA_MLA_PREFILL_SPLIT_MAX_PIECES, plan->rows, split->workspace, split->workspaceBytes, sizeEntry,
                                        &plan->planned, &plan->pieces);
  if (st != MFA_OK) return st;
  if ((uint64_t)plan->blocks * plan->pieces > 0x7FFFFFFFull)
    return fail(MFA_ERR_INVALID_ARGUMENT, "blocks x batches x pieces must fit a grid of 2^31 - 1 workgroups");
  return MFA_OK;
}

// ---- sparse decode (include/mfa_mla_sparse.h, mfa_mla_sparse_fp8.h): one plan over the kernels of the unit that runs it.  The order of
// the refusals is the headers': the sparse block; `e4m3`: the quant block; everything the dense launch refuses for these params, in its
// words; then the grid and the workspace.  The packing is by (sequence, row, group of heads) and the plan is over the slots of a list.
struct MlaSparsePlan : MlaCutPlan<MlaSparseArgs, MLA_LDS> {
  typedef MlaKernelSet<MlaSparseArgs> Set;
  mfa_status prepare(const Set (&sets)[2], bool e4m3, const mfa_mla_decode_params *p, const mfa_mla_sparse *s, const mfa_mla_quant *quant) {
    mfa_status st = check_mla_sparse(s, kMlaDenseDecode);
    if (st == MFA_OK && e4m3) st = check_mla_decode_quant(quant);
    uint32_t pageShift = 0;
    if (st == MFA_OK) st = check_mla_decode_params(p, e4m3, &pageShift);
    if (st != MFA_OK) return st;
    const uint64_t groups = ((uint64_t)p->heads + MFA_MLA_PACKED_ROWS - 1) / MFA_MLA_PACKED_ROWS;
    const uint64_t wide = groups * p->rows * p->batches;
    if (wide * MFA_DECODE_MAX_PIECES > 0x7FFFFFFFull)
      return fail(MFA_ERR_INVALID_ARGUMENT, "groups x rows x batches x pieces must fit a grid of 2^31 - 1 workgroups");
    set = find_mla_set(sets, p->precision);
    blocks = (uint32_t)wide;
    rows = (uint64_t)p->batches * p->heads * p->rows;
    std::memset(&args, 0, sizeof(args));
    MlaArgs &a = args.a;
    fill_mla_args(a, p, pageShift);
    a.M = p->heads * p->rows; a.groups = (uint32_t)groups;
    const uint64_t tiles = ((uint64_t)s->topk + MFA_DECODE_KEY_TILE - 1) / MFA_DECODE_KEY_TILE;
    st = plan_mla_pieces(a, p->pieces, blocks, tiles, MFA_DECODE_WORKGROUP_TARGET, 4, MFA_DECODE_MAX_PIECES, rows, p->workspace, p->workspaceBytes,
                         e4m3 ? "mfa_attention_mla_sparse_decode_fp8_workspace_size" : "mfa_attention_mla_sparse_decode_workspace_size", &planned,
                         &pieces);
    if (st != MFA_OK) return st;
    a.pieces = pieces;
    if (e4m3) a.kvScale = quant->kvScale;
    args.indices = s->indices;
    args.irs = s->indexRowStride;
    args.ibs = s->indexBatchStride;
    args.topk = s->topk;
    return MFA_OK;
  }
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args.a, args.a.kvScale, q, kv, o, l); }
};

// ---- the bodies of the entries.  Plan: prepare(what...), bind(q, kv, o, l), run(stream) and name(), the kernel a HIP failure is
// reported under.  mla_run and mla_time_run are the halves after prepare, for the split entries, which look at a prepared plan first.

template <typename Plan> mfa_status mla_run(Plan &plan, const void *q, const void *kv, void *o, float *l, void *stream) {
  const mfa_status st = plan.bind(q, kv, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}
template <typename Plan, typename... What>
mfa_status mla_launch(const void *q, const void *kv, void *o, float *l, void *stream, const What &...what) {
  Plan plan;
  const mfa_status st = plan.prepare(what...);
  return st != MFA_OK ? st : mla_run(plan, q, kv, o, l, stream);
}

// (the caller has judged the timing arguments)
template <typename Plan>
mfa_status mla_time_run(Plan &plan, const void *q, const void *kv, void *o, float *l, void *stream, int warmup, int iterations, float *milliseconds) {
  const mfa_status st = plan.bind(q, kv, o, l);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}
template <typename Plan, typename... What>
mfa_status mla_time(const void *q, const void *kv, void *o, float *l, void *stream, int warmup, int iterations, float *milliseconds, const What &...what) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  Plan plan;
  const mfa_status st = plan.prepare(what...);
  return st != MFA_OK ? st : mla_time_run(plan, q, kv, o, l, stream, warmup, iterations, milliseconds);
}

// what a workspace_size entry answers from a prepared plan: the bytes `planned` pieces need (unsplit: none), and the pieces.  (An
// entry that has not judged a NULL `bytes` ahead of its plan has it judged here, after it.)
template <typename Plan> mfa_status mla_workspace_answer(const Plan &plan, uint64_t *bytes, uint32_t *pieces) {
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (plan.planned > 1) *bytes = split_workspace_bytes(plan.planned, plan.rows, MLA_DV);
  if (pieces) *pieces = plan.planned;
  return MFA_OK;
}

// workspace_size over a `holder` -- decode's params, prefill's split block -- that may already name a workspace, which is not looked
// at: the plan is prepared from a copy without one.  `prepare(plan, copy or null)` is the family's call of Plan::prepare.
template <typename Plan, typename Holder, typename Prepare>
mfa_status mla_workspace_size(const Holder *holder, uint64_t *bytes, uint32_t *pieces, Prepare prepare) {
  Holder probe;
  if (holder) {
    probe = *holder;
    probe.workspace = nullptr;
    probe.workspaceBytes = 0;
  }
  Plan plan;
  const mfa_status st = prepare(plan, holder ? &probe : nullptr);
  return st != MFA_OK ? st : mla_workspace_answer(plan, bytes, pieces);
}

// ---- the launch forms more than one entry speaks

inline std::string mla_unsplit_note(uint32_t planned) {
  return planned > 1 ? ", unsplit without a workspace: the plan has " + std::to_string(planned) + " pieces" : "";
}

// sparse decode, 16-bit and e4m3
inline void mla_sparse_decode_form(const MlaSparsePlan &plan, char *out, size_t capacity) {
  const MlaArgs &a = plan.args.a;
  const char *layout = a.paged ? "paged" : "contiguous";
  char text[512];
  if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u groups x %u rows x %u sequences x %u pieces, topk %u, %s) + %s (grid %llu)", plan.name(),
                  plan.blocks * plan.pieces, a.groups, a.R, a.batches, plan.pieces, plan.args.topk, layout, plan.set->combine.name,
                  (unsigned long long)combine_grid(plan.rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u = %u groups x %u rows x %u sequences, topk %u, %s%s)", plan.name(), plan.blocks, a.groups, a.R,
                  a.batches, plan.args.topk, layout, mla_unsplit_note(plan.planned).c_str());
  copy_text(out, capacity, text);
}

// prefill, unsplit and cut; `cache`: "" or what an e4m3 cache adds ahead of the layout.  `combine`: the combine kernel of a cut launch.
inline void mla_prefill_form(const char *name, const MlaPrefillArgs &a, uint32_t blocks, uint32_t pieces, uint32_t planned, uint64_t rows,
                             const char *cache, const char *combine, char *out, size_t capacity) {
  const char *layout = a.paged ? "paged" : "contiguous";
  char text[512];
  if (pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u blocks x %u sequences x %u pieces, %llu packed rows in blocks of %d, %s%s) + %s (grid %llu)", name,
                  blocks * pieces, a.blocks, a.batches, pieces, (unsigned long long)a.R * a.H, MFA_MLA_PREFILL_PACKED_ROWS, cache, layout, combine,
                  (unsigned long long)combine_grid(rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u = %u blocks x %u sequences, %llu packed rows in blocks of %d, %s%s%s)", name, blocks, a.blocks,
                  a.batches, (unsigned long long)a.R * a.H, MFA_MLA_PREFILL_PACKED_ROWS, cache, layout, mla_unsplit_note(planned).c_str());
  copy_text(out, capacity, text);
}

} // namespace mfa
