// attn_prefill16.hip -- prefill attention over a KV cache: the kernels' code objects, the C ABI of include/mfa_prefill.h and the prefill
// entries of include/mfa_window.h (a sliding window: the same checks and grid, the attn_prefill16w_* kernels) and of include/mfa_sink.h
// (attention sinks: the attn_prefill16s_* kernels), the prefill entries of include/mfa_ragged.h (packed rows: attn_prefill16r_*) and
// those of include/mfa_softcap.h (a soft cap on the scores: attn_prefill16c_*, over packed rows attn_prefill16rc_*) and those of
// include/mfa_tree.h (a speculation tree among the new rows: attn_prefill16t_*) and those of include/mfa_split.h (the launch cut along
// the keys: attn_prefill16sk_* / attn_prefill16tk_* and the combine kernels attn_prefill16_combine_*).
// The refusals of a window and of sinks, the Sinks of a launch and the host side of the cut along the keys (the piece count's formula, the
// workspace, its check and slabs, the two kernels of a run) are cache_launch.h's, shared with attn_decode16.hip.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_prefill.h"
#include "../../include/mfa_ragged.h"
#include "../../include/mfa_sink.h"
#include "../../include/mfa_softcap.h"
#include "../../include/mfa_split.h"
#include "../../include/mfa_tree.h"
#include "../../include/mfa_window.h"
#include "attn_prefill16.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_prefill16_d<D>_<type>[_e4m3], and attn_prefill16w_*
// under a sliding window, attn_prefill16s_* with attention sinks, attn_prefill16r_* over packed rows (the sink body: one ragged kernel
// serves plain, window and sink launches), attn_prefill16c_* / attn_prefill16rc_* with a soft cap (the sink body and the ragged one),
// attn_prefill16t_* with a speculation tree (the sink body), attn_prefill16sk_* / attn_prefill16tk_* cut along the keys (the sink and the
// tree body), whose pieces attn_prefill16_combine_d<D>_<type> merges
// (the macros that generate them from one list of families: attn_prefill16.h).  D = 256 lives in attn_prefill16_d256.hip.
MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, bf16, __bf16, 64)
MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, bf16, __bf16, 128)
MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, f16, _Float16, 64)
MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, f16, _Float16, 128)
MFA_PREFILL_KERNELS(MFA_PREFILL_DECLARE, bf16, __bf16, 256)
MFA_PREFILL_KERNELS(MFA_PREFILL_DECLARE, f16, _Float16, 256)
MFA_PREFILL_COMBINE_DEFINE(bf16, __bf16, 64)
MFA_PREFILL_COMBINE_DEFINE(bf16, __bf16, 128)
MFA_PREFILL_COMBINE_DEFINE(f16, _Float16, 64)
MFA_PREFILL_COMBINE_DEFINE(f16, _Float16, 128)
MFA_PREFILL_COMBINE_DECLARE(bf16, __bf16, 256)
MFA_PREFILL_COMBINE_DECLARE(f16, _Float16, 256)

namespace {

// the families of MFA_PREFILL_FAMILIES by their kernels' infix -- F_: plain, F_w: window, F_s: sinks, F_r: ragged, F_c / F_rc: padded /
// ragged with a soft cap, F_t: tree, F_sk / F_tk: sinks / tree cut along the keys -- and their count: the kernels' first index, generated
// from the list that generates the kernels
#define MFA_PREFILL_FAMILY_ID(K, I, ...) F_##I,
enum Family { MFA_PREFILL_FAMILIES(MFA_PREFILL_FAMILY_ID, , , , ) FAMILIES };
typedef CacheKernel<PrefillArgs> PrefillKernel;
struct PrefillSet {
  uint32_t D;
  int precision;
  uint32_t lds;
  PrefillKernel kernel[FAMILIES][2];   // [family][e4m3]
  PrefillKernel combine;               // merges the pieces of F_sk and F_tk
};
#define MFA_PREFILL_SET_FAMILY(K, I, WINDOW, SINK, RAGGED, CAP, TREE, SPLIT, TN, T, D)                                                          \
  {MFA_CACHE_KERNEL(attn_prefill16##I##_d##D##_##TN), MFA_CACHE_KERNEL(attn_prefill16##I##_d##D##_##TN##_e4m3)},
#define MFA_PREFILL_SET(TN, PREC, D)                                                                                                  \
  {D, PREC, (uint32_t)prefill16_lds_bytes<D>(), {MFA_PREFILL_FAMILIES(MFA_PREFILL_SET_FAMILY, , TN, , D)},                            \
   MFA_CACHE_KERNEL(attn_prefill16_combine_d##D##_##TN)}
const PrefillSet kSets[] = {MFA_PREFILL_SET(bf16, MFA_BF16, 64), MFA_PREFILL_SET(bf16, MFA_BF16, 128), MFA_PREFILL_SET(bf16, MFA_BF16, 256),
                            MFA_PREFILL_SET(f16, MFA_FP16, 64),  MFA_PREFILL_SET(f16, MFA_FP16, 128),  MFA_PREFILL_SET(f16, MFA_FP16, 256)};

// min(T / RB + batches, batches x ceil(rows / RB)): never below sum_b ceil(qn_b / RB) for non-decreasing starts
uint64_t ragged_slots(uint32_t totalRows, uint32_t batches, uint32_t rows, uint32_t RB) {
  const uint64_t tight = (uint64_t)totalRows / RB + batches, padded = (uint64_t)batches * (((uint64_t)rows + RB - 1) / RB);
  return tight < padded ? tight : padded;
}

// Pieces of the keys (include/mfa_split.h; choose_pieces, cache_launch.h): chosen from the workgroups the launch has without a split and
// planned_tiles.  Aims at MFA_PREFILL_SPLIT_COMPUTE_UNITS x the workgroups per compute unit the kernel's LDS allows (2 at D <= 128, 1 at
// D = 256); a piece keeps at least MFA_PREFILL_SPLIT_MIN_TILES.
struct PrefillPlan {
  PrefillArgs args;
  const PrefillSet *set;
  bool fp8;
  Family family;     // the kernels' first index
  uint32_t blocks;   // batches x K/V heads x row blocks; ragged: slots x K/V heads
  uint32_t pieces;   // as the launch runs: 1 without a split block, without a workspace, or when one piece is asked for or planned
  uint32_t planned;  // what the split block asks for (pieces = 0: the host's plan); 1 without one
  uint64_t rows;     // batches x heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  const PrefillKernel &kernel() const { return set->kernel[family][fp8]; }
  const char *name() const { return kernel().name; }
  mfa_status prepare(const mfa_prefill_params *p, const LaunchOptions &options);
  hipError_t run(hipStream_t stream) const;
};

// every check that needs no GPU, and the kernel's argument block (the buffer pointers are filled in by bind).  options.ragged non-null:
// packed rows, include/mfa_ragged.h
mfa_status PrefillPlan::prepare(const mfa_prefill_params *p, const LaunchOptions &options) {
  const mfa_ragged_rows *ragged = options.ragged;
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (ragged) {
    if (!ragged->rowStarts)
      return fail(MFA_ERR_INVALID_ARGUMENT, "rowStarts is required (device array of batches + 1 uint32: the first packed row of every sequence, and the end of the last)");
    if (ragged->totalRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "totalRows must be non-zero (the packed rows of Q, O and L)");
    if (p->queryLengths)
      return fail(MFA_ERR_INVALID_ARGUMENT, "queryLengths must be NULL for a ragged launch: rowStarts gives every sequence's row count");
    if (p->batchStride[0] != 0 || p->batchStride[3] != 0)
      return fail(MFA_ERR_INVALID_ARGUMENT, "batchStride of Q and O must be 0 for a ragged launch: the packed layout [totalRows][heads][D] has no batch axis");
    if (p->lBatchStride != 0)
      return fail(MFA_ERR_INVALID_ARGUMENT, "lBatchStride must be 0 for a ragged launch: the packed L [heads][totalRows] has no batch axis");
  }
  mfa_status allowed = check_window_and_sinks(options.window, options.sinks, p->causal != 0);
  if (allowed == MFA_OK) allowed = check_softcap(options.softcap);
  if (allowed == MFA_OK) allowed = check_tree(options, p->causal != 0, p->rows, MFA_TREE_MAX_NODES);
  if (allowed != MFA_OK) return allowed;
  const mfa_key_split *split = options.split;
  if (split && split->pieces > MFA_PREFILL_SPLIT_MAX_PIECES)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_key_split.pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64 (a lane of the combine kernel's "
                                          "wave per piece), not " + std::to_string(split->pieces));
  if (split && (ragged || options.softcap != 0.0f))
    return fail(MFA_ERR_UNSUPPORTED, "a key split goes with neither packed rows nor a soft cap: they have no split kernel (include/mfa_split.h)");
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, "prefill attention takes a 16-bit Q (precision MFA_BF16 or MFA_FP16); FP32 Q has no kernel");
  mfa_status st = check_precisions(p->precision, p->outputPrecision);
  if (st == MFA_OK) st = check_cache_precision(p->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8 && p->cachePrecision != p->precision)
    return fail(MFA_ERR_INVALID_ARGUMENT, "cachePrecision must be `precision` (a 16-bit cache of Q's type) or MFA_KV_E4M3");
  if (!fp8 && (p->keyScale || p->valueScale))
    return fail(MFA_ERR_INVALID_ARGUMENT, "keyScale / valueScale go with an e4m3 cache (cachePrecision MFA_KV_E4M3); a 16-bit cache holds the values themselves");
  const PrefillSet *set = nullptr;
  for (const PrefillSet &s : kSets)
    if (s.D == p->headDimension && s.precision == p->precision) set = &s;
  if (!set)
    return fail(MFA_ERR_UNSUPPORTED, "prefill attention is compiled for head dimensions 256, 64 and 128, not " + std::to_string(p->headDimension));
  if ((st = check_sizes(p)) != MFA_OK) return st;
  const uint32_t G = p->headsPerKeyValue > 1 ? p->headsPerKeyValue : 1;
  if (G > MFA_PREFILL_MAX_GROUP)
    return fail(MFA_ERR_UNSUPPORTED, "prefill attention packs the headsPerKeyValue query heads of a K/V head into one workgroup: headsPerKeyValue must be "
                                     "at most 32, not " + std::to_string(G));
  uint32_t pageShift = 0;
  if ((st = check_group(p->heads, G)) != MFA_OK || (st = check_cache_and_strides(p, fp8, &pageShift)) != MFA_OK) return st;
  const uint32_t RB = MFA_PREFILL_PACKED_ROWS / G;
  const uint64_t rowBlocks = ((uint64_t)p->rows + RB - 1) / RB;
  uint64_t blocks = (uint64_t)p->batches * (p->heads / G) * rowBlocks, slots = 0;
  if (ragged) {
    if ((uint64_t)p->batches * rowBlocks > 0x7fffffffull)
      return fail(MFA_ERR_UNSUPPORTED, "batches x ceil(rows / " + std::to_string(RB) + ") = " + std::to_string((uint64_t)p->batches * rowBlocks) +
                                           " row blocks exceed 2^31 - 1: rows is the largest row count of a sequence, not totalRows");
    slots = ragged_slots(ragged->totalRows, p->batches, p->rows, RB);
    blocks = slots * (p->heads / G);
    if (blocks > 0x7fffffffull)
      return fail(MFA_ERR_UNSUPPORTED, "slots x K/V heads = " + std::to_string(blocks) + " workgroups exceed one grid (2^31 - 1)");
  } else if (blocks > 0x7fffffffull)
    return fail(MFA_ERR_UNSUPPORTED, "batches x K/V heads x row blocks = " + std::to_string(blocks) + " workgroups exceed one grid (2^31 - 1)");
  this->set = set;
  family = options.tree ? F_t : options.softcap != 0.0f ? (ragged ? F_rc : F_c) : ragged ? F_r : options.sinks.any() ? F_s : options.window != 0 ? F_w : F_;
  this->blocks = (uint32_t)blocks;
  rows = (uint64_t)p->batches * p->heads * p->rows;
  planned = pieces = 1;
  if (split) {
    planned = split->pieces ? split->pieces
                            : choose_pieces(blocks, planned_tiles(p->column, p->rows, options.window, options.sinks.tokens),
                                            (uint64_t)MFA_PREFILL_SPLIT_COMPUTE_UNITS * (set->D == 256 ? 1 : 2), MFA_PREFILL_SPLIT_MIN_TILES,
                                            MFA_PREFILL_SPLIT_MAX_PIECES);
    pieces = split->workspace ? planned : 1;   // no workspace: one kernel, unsplit
    if (pieces > 1) {
      st = check_split_workspace(split->workspace, split->workspaceBytes, split_workspace_bytes(pieces, rows, set->D), "mfa_attention_prefill_split_workspace_size");
      if (st != MFA_OK) return st;
      if (blocks * pieces > 0x7fffffffull)
        return fail(MFA_ERR_UNSUPPORTED, "batches x K/V heads x row blocks x pieces = " + std::to_string(blocks * pieces) + " workgroups exceed one grid (2^31 - 1)");
      family = options.tree ? F_tk : F_sk;
    }
  }
  PrefillArgs &a = args;
  set_shared_args(a, p, G, pageShift, options);
  if (pieces > 1) {
    a.heads = p->heads;
    set_split_slabs(a, split->workspace, pieces, rows, set->D);
  }
  a.qlengths = p->queryLengths;
  a.keyScale = fp8 ? p->keyScale : nullptr;
  a.valueScale = fp8 ? p->valueScale : nullptr;
  a.rows = p->rows; a.RB = RB; a.rowBlocks = (uint32_t)rowBlocks;
  if (ragged) {
    a.rowStarts = ragged->rowStarts;
    a.totalRows = ragged->totalRows;
    a.slots = (uint32_t)slots;
  }
  return MFA_OK;
}

hipError_t PrefillPlan::run(hipStream_t stream) const {
  static_assert(PF_THREADS == 256, "run_pieces starts workgroups of 256 threads");
  return run_pieces(kernel(), blocks, pieces, set->lds, set->combine, rows, stream, args);
}

mfa_status prefill_launch_form(const mfa_prefill_params *params, const LaunchOptions &options, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  PrefillPlan plan;
  mfa_status st = entry_check(options, !out || capacity == 0 ? "null argument" : nullptr);
  if (st == MFA_OK) st = plan.prepare(params, options);
  if (st != MFA_OK) return st;
  const PrefillArgs &a = plan.args;
  const Sinks &sinks = options.sinks;
  char text[512];
  // (a windowed launch names its window, then its sink tokens; bound sink logits, then the soft cap, then the tree, last)
  char cap[48] = "";
  if (options.softcap != 0.0f) std::snprintf(cap, sizeof(cap), ", softcap %g", (double)options.softcap);
  const std::string tail = (options.window ? ", window " + std::to_string(options.window) : std::string()) +
                           (sinks.tokens ? ", sink tokens " + std::to_string(sinks.tokens) : std::string()) + (sinks.logits ? ", sink logits" : "") + cap +
                           tree_form(options);
  if (options.ragged)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u slots x %u K/V heads, row blocks of %u rows x %u heads, %u packed rows of %u sequences, at most %u rows each, %s%s)",
                  plan.name(), plan.blocks, a.slots, a.Hkv, a.RB, a.G, a.totalRows, a.batches, a.rows, a.paged ? "paged" : "contiguous", tail.c_str());
  else if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u sequences x %u K/V heads x %u row blocks of %u rows x %u heads x %u pieces%s, %s%s) + %s (grid %u)",
                  plan.name(), plan.blocks * plan.pieces, a.batches, a.Hkv, a.rowBlocks, a.RB, a.G, plan.pieces,
                  options.split->pieces ? " as given" : "", a.paged ? "paged" : "contiguous", tail.c_str(), plan.set->combine.name, (uint32_t)combine_grid(plan.rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u = %u sequences x %u K/V heads x %u row blocks of %u rows x %u heads, %s%s%s)", plan.name(),
                  plan.blocks, a.batches, a.Hkv, a.rowBlocks, a.RB, a.G, a.paged ? "paged" : "contiguous", tail.c_str(),
                  plan.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces").c_str() : "");
  copy_text(out, capacity, text);
  return MFA_OK;
}

// the bytes of the workspace the launch would split into and the piece count: 0 and 1 for an unsplit plan, whatever workspace the
// block may already name
mfa_status prefill_split_workspace_size(const mfa_prefill_params *params, const LaunchOptions &options, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 1;
  const mfa_status refused = entry_check(options, !bytes ? "null argument" : nullptr);
  if (refused != MFA_OK) return refused;
  mfa_key_split probe = *options.split;
  probe.workspace = nullptr;
  probe.workspaceBytes = 0;
  LaunchOptions probed = options;
  probed.split = &probe;
  PrefillPlan plan;
  const mfa_status st = plan.prepare(params, probed);
  if (st != MFA_OK) return st;
  if (plan.planned > 1) *bytes = split_workspace_bytes(plan.planned, plan.rows, plan.set->D);
  if (pieces) *pieces = plan.planned;
  return MFA_OK;
}

constexpr auto prefill_launch = cache_launch<PrefillPlan, mfa_prefill_params>;
constexpr auto prefill_time = cache_time<PrefillPlan, mfa_prefill_params>;

} // namespace

extern "C" {

void mfa_prefill_params_init(mfa_prefill_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->outputPrecision = MFA_BF16;
  params->cachePrecision = MFA_BF16;
  params->headsPerKeyValue = 1;
  params->causal = 1;
}

size_t mfa_prefill_params_size(void) { return sizeof(mfa_prefill_params); }

mfa_status mfa_prefill_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_OFF(f) (uint32_t)offsetof(mfa_prefill_params, f)
  static const uint32_t table[] = {
      MFA_OFF(rows), MFA_OFF(column), MFA_OFF(heads), MFA_OFF(batches), MFA_OFF(headsPerKeyValue), MFA_OFF(causal), MFA_OFF(headDimension),
      MFA_OFF(precision), MFA_OFF(outputPrecision), MFA_OFF(pageSize), MFA_OFF(cacheLengths), MFA_OFF(queryLengths), MFA_OFF(blockTable),
      MFA_OFF(blockTableStride), MFA_OFF(leadingDimension), MFA_OFF(headStride), MFA_OFF(batchStride), MFA_OFF(pageStride),
      MFA_OFF(lHeadStride), MFA_OFF(lBatchStride), MFA_OFF(cachePrecision), MFA_OFF(reserved), MFA_OFF(keyScale), MFA_OFF(valueScale)};
#undef MFA_OFF
  const uint32_t total = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = total;
  for (uint32_t i = 0; i < total && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_prefill_tile_range(uint32_t length, uint32_t queryLength, uint32_t firstRow, uint32_t blockRows, uint32_t causal,
                                            uint32_t *firstMasked, uint32_t *end) {
  if (!firstMasked || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (blockRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "blockRows must be non-zero");
  prefill_tile_range(length, queryLength, firstRow, blockRows, causal, firstMasked, end);
  return MFA_OK;
}

mfa_status mfa_attention_prefill_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                        void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions(), stream);
}

mfa_status mfa_attention_prefill_launch_form(const mfa_prefill_params *params, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions(), out, capacity);
}

mfa_status mfa_attention_prefill_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                      void *stream, int warmup, int iterations, float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions(), stream, warmup, iterations, milliseconds);
}

// ---- under a sliding window (include/mfa_window.h): the same three with `window` after `params`; window 0 is the launch without one

mfa_status mfa_attention_prefill_window_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                               uint32_t window, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window), stream);
}

mfa_status mfa_attention_prefill_window_launch_form(const mfa_prefill_params *params, uint32_t window, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window), out, capacity);
}

mfa_status mfa_attention_prefill_window_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                             uint32_t window, void *stream, int warmup, int iterations, float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_prefill_window_tile_range(uint32_t length, uint32_t queryLength, uint32_t firstRow, uint32_t blockRows, uint32_t window,
                                                   uint32_t *begin, uint32_t *unmaskedBegin, uint32_t *unmaskedEnd, uint32_t *end) {
  if (!begin || !unmaskedBegin || !unmaskedEnd || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (blockRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "blockRows must be non-zero");
  if (window == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "window must be non-zero (no window: mfa_attention_prefill_tile_range)");
  prefill_window_tile_range(length, queryLength, firstRow, blockRows, window, begin, unmaskedBegin, unmaskedEnd, end);
  return MFA_OK;
}

// ---- with attention sinks (include/mfa_sink.h): the window entries with `sinks` after `window`.  The block is required; an all-zero
// one is the window launch, whichever window

mfa_status mfa_attention_prefill_sink_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                             uint32_t window, const mfa_attention_sinks *sinks, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window).required_sinks(sinks), stream);
}

mfa_status mfa_attention_prefill_sink_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks, char *out,
                                                  size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window).required_sinks(sinks), out, capacity);
}

mfa_status mfa_attention_prefill_sink_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                           uint32_t window, const mfa_attention_sinks *sinks, void *stream, int warmup, int iterations,
                                           float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window).required_sinks(sinks), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_prefill_sink_tile_range(uint32_t length, uint32_t queryLength, uint32_t firstRow, uint32_t blockRows, uint32_t causal,
                                                 uint32_t window, uint32_t sinkTokens, uint32_t *begin, uint32_t *unmaskedBegin,
                                                 uint32_t *unmaskedEnd, uint32_t *end, uint32_t *sinkEnd) {
  if (!begin || !unmaskedBegin || !unmaskedEnd || !end || !sinkEnd) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (blockRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "blockRows must be non-zero");
  if (window && !causal) return fail(MFA_ERR_INVALID_ARGUMENT, "a sliding window needs causal");
  if (sinkTokens && !window) return fail(MFA_ERR_INVALID_ARGUMENT, "sink tokens need a window: sinkTokens must be 0 when window is 0");
  prefill_sink_tile_range(length, queryLength, firstRow, blockRows, causal, window, sinkTokens, begin, unmaskedBegin, unmaskedEnd, end, sinkEnd);
  return MFA_OK;
}

// ---- over packed rows (include/mfa_ragged.h): the sink entries with `ragged` after `sinks`; a NULL `sinks` is no sinks

void mfa_ragged_rows_init(mfa_ragged_rows *ragged) {
  if (ragged) std::memset(ragged, 0, sizeof(*ragged));
}

size_t mfa_ragged_rows_size(void) { return sizeof(mfa_ragged_rows); }

mfa_status mfa_ragged_rows_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  static const uint32_t table[] = {(uint32_t)offsetof(mfa_ragged_rows, rowStarts), (uint32_t)offsetof(mfa_ragged_rows, totalRows),
                                   (uint32_t)offsetof(mfa_ragged_rows, reserved)};
  *count = 3;
  for (uint32_t i = 0; i < 3 && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_prefill_ragged_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                               uint32_t window, const mfa_attention_sinks *sinks, const mfa_ragged_rows *ragged, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).ragged_of(ragged), stream);
}

mfa_status mfa_attention_prefill_ragged_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                    const mfa_ragged_rows *ragged, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window).optional_sinks(sinks).ragged_of(ragged), out, capacity);
}

mfa_status mfa_attention_prefill_ragged_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                             uint32_t window, const mfa_attention_sinks *sinks, const mfa_ragged_rows *ragged, void *stream,
                                             int warmup, int iterations, float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).ragged_of(ragged), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_prefill_ragged_slots(uint32_t totalRows, uint32_t batches, uint32_t rows, uint32_t blockRows, uint64_t *slots) {
  if (!slots) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (blockRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "blockRows must be non-zero");
  *slots = ragged_slots(totalRows, batches, rows, blockRows);
  return MFA_OK;
}

mfa_status mfa_attention_prefill_ragged_block(const uint32_t *rowStarts, uint32_t batches, uint32_t totalRows, uint32_t rows, uint32_t blockRows,
                                              uint32_t slot, uint32_t *sequence, uint32_t *firstRow) {
  if (!rowStarts || !sequence || !firstRow) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (blockRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "blockRows must be non-zero");
  uint32_t start, count;
  prefill_ragged_block(rowStarts, batches, totalRows, rows, blockRows, slot, sequence, firstRow, &start, &count);
  return MFA_OK;
}

// ---- with a soft cap (include/mfa_softcap.h): the sink entries with `softcap` after `sinks`, the ragged entries with it after
// `ragged`; a NULL `sinks` is no sinks.  softcap 0 is the launch of the headers below, whichever window, sinks and rows

mfa_status mfa_attention_prefill_softcap_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                                uint32_t window, const mfa_attention_sinks *sinks, float softcap, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).capped(softcap), stream);
}

mfa_status mfa_attention_prefill_softcap_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                     float softcap, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window).optional_sinks(sinks).capped(softcap), out, capacity);
}

mfa_status mfa_attention_prefill_softcap_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                              uint32_t window, const mfa_attention_sinks *sinks, float softcap, void *stream, int warmup,
                                              int iterations, float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).capped(softcap), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_prefill_ragged_softcap_launch(const void *q, const void *k, const void *v, void *o, float *l,
                                                       const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                       const mfa_ragged_rows *ragged, float softcap, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).ragged_of(ragged).capped(softcap), stream);
}

mfa_status mfa_attention_prefill_ragged_softcap_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                            const mfa_ragged_rows *ragged, float softcap, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window).optional_sinks(sinks).ragged_of(ragged).capped(softcap), out, capacity);
}

mfa_status mfa_attention_prefill_ragged_softcap_time(const void *q, const void *k, const void *v, void *o, float *l,
                                                     const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                     const mfa_ragged_rows *ragged, float softcap, void *stream, int warmup, int iterations,
                                                     float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).ragged_of(ragged).capped(softcap), stream, warmup, iterations, milliseconds);
}

// ---- with a speculation tree (include/mfa_tree.h): the sink entries with `tree` after `sinks`; a NULL `sinks` is no sinks, the tree
// block is required (mfa_attention_tree_init and its size / offsets: attn_decode16.hip)

mfa_status mfa_attention_prefill_tree_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                             uint32_t window, const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).tree_of(tree), stream);
}

mfa_status mfa_attention_prefill_tree_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                  const mfa_attention_tree *tree, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window).optional_sinks(sinks).tree_of(tree), out, capacity);
}

mfa_status mfa_attention_prefill_tree_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                           uint32_t window, const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, void *stream,
                                           int warmup, int iterations, float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).tree_of(tree), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_prefill_tree_tile_range(uint32_t length, uint32_t queryLength, uint32_t window, uint32_t sinkTokens, uint32_t *begin,
                                                 uint32_t *unmaskedBegin, uint32_t *unmaskedEnd, uint32_t *end, uint32_t *sinkEnd) {
  if (!begin || !unmaskedBegin || !unmaskedEnd || !end || !sinkEnd) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (sinkTokens && !window) return fail(MFA_ERR_INVALID_ARGUMENT, "sink tokens need a window: sinkTokens must be 0 when window is 0");
  prefill_tree_tile_range(length, queryLength, window, sinkTokens, begin, unmaskedBegin, unmaskedEnd, end, sinkEnd);
  return MFA_OK;
}

// ---- cut along the keys (include/mfa_split.h): the tree entries with `split` after `tree`; NULL `sinks` and NULL `tree` are none, the
// split block is required

void mfa_key_split_init(mfa_key_split *split) {
  if (split) std::memset(split, 0, sizeof(*split));
}

size_t mfa_key_split_size(void) { return sizeof(mfa_key_split); }

mfa_status mfa_key_split_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  static const uint32_t table[] = {(uint32_t)offsetof(mfa_key_split, workspace), (uint32_t)offsetof(mfa_key_split, workspaceBytes),
                                   (uint32_t)offsetof(mfa_key_split, pieces), (uint32_t)offsetof(mfa_key_split, reserved)};
  *count = 4;
  for (uint32_t i = 0; i < 4 && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_prefill_split_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                              uint32_t window, const mfa_attention_sinks *sinks, const mfa_attention_tree *tree,
                                              const mfa_key_split *split, void *stream) {
  return prefill_launch(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).optional_tree(tree).split_of(split), stream);
}

mfa_status mfa_attention_prefill_split_launch_form(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                   const mfa_attention_tree *tree, const mfa_key_split *split, char *out, size_t capacity) {
  return prefill_launch_form(params, LaunchOptions().within(window).optional_sinks(sinks).optional_tree(tree).split_of(split), out, capacity);
}

mfa_status mfa_attention_prefill_split_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_prefill_params *params,
                                            uint32_t window, const mfa_attention_sinks *sinks, const mfa_attention_tree *tree,
                                            const mfa_key_split *split, void *stream, int warmup, int iterations, float *milliseconds) {
  return prefill_time(q, k, v, o, l, params, LaunchOptions().within(window).optional_sinks(sinks).optional_tree(tree).split_of(split), stream, warmup,
                      iterations, milliseconds);
}

mfa_status mfa_attention_prefill_split_workspace_size(const mfa_prefill_params *params, uint32_t window, const mfa_attention_sinks *sinks,
                                                      const mfa_attention_tree *tree, const mfa_key_split *split, uint64_t *bytes,
                                                      uint32_t *pieces) {
  return prefill_split_workspace_size(params, LaunchOptions().within(window).optional_sinks(sinks).optional_tree(tree).split_of(split), bytes, pieces);
}

mfa_status mfa_attention_prefill_split_piece_range(uint32_t beginTile, uint32_t endTile, uint32_t sinkEnd, uint32_t pieces, uint32_t piece,
                                                   uint32_t begin[2], uint32_t end[2]) {
  if (!begin || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, pieces non-zero");
  if (sinkEnd > beginTile || beginTile > endTile)
    return fail(MFA_ERR_INVALID_ARGUMENT, "the walked list is [0, sinkEnd) ++ [beginTile, endTile): sinkEnd <= beginTile <= endTile");
  prefill_split_piece_range(beginTile, endTile, sinkEnd, pieces, piece, begin, end);
  return MFA_OK;
}

} // extern "C"
