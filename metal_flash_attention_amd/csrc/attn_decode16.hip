// attn_decode16.hip -- decode attention over a KV cache, 16-bit or FP8 (e4m3): the kernels' code objects, the C ABI of
// include/mfa_decode.h, the decode entries of include/mfa_kvcache.h and those of include/mfa_window.h (a sliding window: the same
// plan with the piece count taken from the tiles a window can span, and the attn_decode16w_* / attn_decode8w_* kernels) and those of
// include/mfa_sink.h (attention sinks: the window's plan plus the sink tiles, and the attn_decode16s_* / attn_decode8s_* kernels) and
// those of include/mfa_softcap.h (a soft cap on the scores: the sink launch's plan, and the attn_decode16c_* / attn_decode8c_* kernels) and
// those of include/mfa_tree.h (a speculation tree among the new rows: the sink launch's plan again, and attn_decode16t_* / attn_decode8t_*).  One
// plan serves both: the launch over an e4m3 cache adds its own checks in front of the 16-bit launch's, starts the attn_decode8_*
// kernels in place of _single / _pieces, and shares the piece count, the workspace formula and the combine kernel.  The refusals of a
// window and of sinks, the Sinks of a launch and the host side of the cut along the keys (the piece count's formula, the workspace, its
// check and slabs, the two kernels of a run) are cache_launch.h's, shared with attn_prefill16.hip.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_decode.h"
#include "../../include/mfa_kvcache.h"
#include "../../include/mfa_sink.h"
#include "../../include/mfa_softcap.h"
#include "../../include/mfa_tree.h"
#include "../../include/mfa_window.h"
#include "attn_decode16.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_decode16_d<D>_<type>_{single,pieces,combine} and, over
// an e4m3 cache, attn_decode8_d<D>_<type of Q>_{single,pieces}, whose pieces attn_decode16_d<D>_<type>_combine merges; under a
// sliding window attn_decode16w_* / attn_decode8w_*, with attention sinks attn_decode16s_* / attn_decode8s_*, with a soft cap (whatever
// the window and sinks) attn_decode16c_* / attn_decode8c_*, with a speculation tree attn_decode16t_* / attn_decode8t_*, merged by the same
// combine kernel
// (the macros that generate them from one list of families: attn_decode16.h).  D = 256 lives in attn_decode16_d256.hip.
MFA_DECODE_KERNELS(MFA_DECODE_DEFINE, bf16, __bf16, 64)
MFA_DECODE_KERNELS(MFA_DECODE_DEFINE, bf16, __bf16, 128)
MFA_DECODE_KERNELS(MFA_DECODE_DEFINE, f16, _Float16, 64)
MFA_DECODE_KERNELS(MFA_DECODE_DEFINE, f16, _Float16, 128)
MFA_DECODE_KERNELS(MFA_DECODE_DECLARE, bf16, __bf16, 256)
MFA_DECODE_KERNELS(MFA_DECODE_DECLARE, f16, _Float16, 256)

namespace {

// the families of MFA_DECODE_FAMILIES by their kernels' infix -- F_: plain, F_w: window, F_s: sinks, F_c: soft cap, F_t: tree (both
// whatever the window and sinks) -- and their count: the kernels' first index, generated from the list that generates the kernels
#define MFA_DECODE_FAMILY_ID(K, I, ...) F_##I,
enum Family { MFA_DECODE_FAMILIES(MFA_DECODE_FAMILY_ID, , , , ) FAMILIES };
typedef CacheKernel<DecodeArgs> DecodeKernel;
struct DecodeSet {
  uint32_t D;
  int precision;
  uint32_t lds;
  DecodeKernel kernel[FAMILIES][2][2];   // [family][fp8][pieces]
  DecodeKernel combine;
};
#define MFA_DECODE_SET_FAMILY(K, I, WINDOW, SINK, CAP, TREE, TN, T, D)                                                                     \
  {{MFA_CACHE_KERNEL(attn_decode16##I##_d##D##_##TN##_single), MFA_CACHE_KERNEL(attn_decode16##I##_d##D##_##TN##_pieces)},            \
   {MFA_CACHE_KERNEL(attn_decode8##I##_d##D##_##TN##_single), MFA_CACHE_KERNEL(attn_decode8##I##_d##D##_##TN##_pieces)}},
#define MFA_DECODE_SET(TN, PREC, D)                                                                                                   \
  {D, PREC, (uint32_t)decode16_lds_bytes<D>(), {MFA_DECODE_FAMILIES(MFA_DECODE_SET_FAMILY, , TN, , D)},                               \
   MFA_CACHE_KERNEL(attn_decode16_d##D##_##TN##_combine)}
const DecodeSet kSets[] = {MFA_DECODE_SET(bf16, MFA_BF16, 64), MFA_DECODE_SET(bf16, MFA_BF16, 128), MFA_DECODE_SET(bf16, MFA_BF16, 256),
                           MFA_DECODE_SET(f16, MFA_FP16, 64),  MFA_DECODE_SET(f16, MFA_FP16, 128),  MFA_DECODE_SET(f16, MFA_FP16, 256)};

// Pieces of the keys (choose_pieces, cache_launch.h): chosen from the workgroups the launch has without a split (batches x K/V heads) and
// planned_tiles of `column`.  Aims at MFA_DECODE_WORKGROUP_TARGET workgroups (two per compute unit of a 256-CU chip, what choose_splits
// of mfa_kernel.hip aims at); a piece keeps at least four 64-key tiles (two steps for each of the workgroup's four waves).
struct DecodePlan {
  DecodeArgs args;
  const DecodeSet *set;
  bool fp8;
  Family family;        // the kernels' first index
  uint64_t tiles;       // what the piece count was chosen from
  uint32_t pieces;      // as the launch runs: 1 without a workspace
  uint32_t planned;     // what the host would cut the keys into
  uint32_t blocks;      // batches x K/V heads
  uint64_t rows;        // batches x query heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  // the kernel that reads the cache; its name is what a HIP failure is reported under
  const DecodeKernel &kernel() const { return set->kernel[family][fp8][pieces > 1]; }
  const char *name() const { return kernel().name; }
  mfa_status prepare(const mfa_decode_params *p, const LaunchOptions &options);
  hipError_t run(hipStream_t stream) const;
};

// every check that needs no GPU, and the kernel's argument block (the buffer pointers are filled in by bind).  options.quant is null for
// a 16-bit cache; an e4m3 cache puts its own checks first, then the 16-bit launch's
mfa_status DecodePlan::prepare(const mfa_decode_params *p, const LaunchOptions &options) {
  const mfa_kv_quant *quant = options.quant;
  const uint32_t window = options.window;
  const Sinks &sinks = options.sinks;
  const float softcap = options.softcap;
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_status allowed = check_window_and_sinks(window, sinks, p->causal != 0);
  if (allowed == MFA_OK) allowed = check_softcap(softcap);
  if (allowed == MFA_OK) allowed = check_tree(options, p->causal != 0, p->rows, 0);   // (rows: G x rows <= 32 below)
  if (allowed != MFA_OK) return allowed;
  if (quant) {
    bool e4m3;
    const mfa_status st = check_cache_precision(quant->cachePrecision, &e4m3);
    if (st != MFA_OK) return st;
    if (!e4m3)
      return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_kv_quant.cachePrecision must be MFA_KV_E4M3 (16-bit caches: mfa_attention_decode_launch)");
    if (p->precision == MFA_FP32)
      return fail(MFA_ERR_UNSUPPORTED, "decode attention over an e4m3 cache takes a 16-bit Q (precision MFA_BF16 or MFA_FP16); FP32 Q has no kernel");
    for (int i = 1; i <= 2; ++i) {
      const mfa_status ok = check_stride_multiples(i == 1 ? "K" : "V", p->leadingDimension[i], p->headStride[i],
                                                   p->pageSize ? p->pageStride[i - 1] : p->batchStride[i], 16, "(16-byte rows of an e4m3 cache)");
      if (ok != MFA_OK) return ok;
    }
  }
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention reads 16-bit caches (MFA_BF16 or MFA_FP16); an FP32 cache has no kernel");
  mfa_status st = check_precisions(p->precision, p->outputPrecision);
  if (st != MFA_OK) return st;
  const DecodeSet *set = nullptr;
  for (const DecodeSet &s : kSets)
    if (s.D == p->headDimension && s.precision == p->precision) set = &s;
  if (!set)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention is compiled for head dimensions 256, 64 and 128, not " + std::to_string(p->headDimension));
  if ((st = check_sizes(p)) != MFA_OK) return st;
  const uint32_t G = p->headsPerKeyValue > 1 ? p->headsPerKeyValue : 1;
  if ((st = check_group(p->heads, G)) != MFA_OK) return st;
  if ((uint64_t)G * p->rows > MFA_DECODE_MAX_PACKED_ROWS)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention packs headsPerKeyValue x rows = " + std::to_string((uint64_t)G * p->rows) +
                                         " rows into one tile of at most 32; a longer block of query rows is a prefill: use "
                                         "mfa_attention_kernel_launch with headsPerKeyValue, columnLengths and causal");
  uint32_t pageShift = 0;
  if ((st = check_cache_and_strides(p, false, &pageShift)) != MFA_OK) return st;
  this->set = set;
  fp8 = quant != nullptr;
  blocks = p->batches * (p->heads / G);
  rows = (uint64_t)p->batches * p->heads * p->rows;
  family = options.tree ? F_t : softcap != 0.0f ? F_c : sinks.any() ? F_s : window != 0 ? F_w : F_;
  tiles = planned_tiles(p->column, p->rows, window, sinks.tokens);
  planned = choose_pieces(blocks, tiles, MFA_DECODE_WORKGROUP_TARGET, 4, MFA_DECODE_MAX_PIECES);
  pieces = planned;
  if (!p->workspace) pieces = 1;   // no workspace: one kernel, unsplit
  if (pieces > 1) {
    st = check_split_workspace(p->workspace, p->workspaceBytes, split_workspace_bytes(pieces, rows, set->D), "mfa_attention_decode_workspace_size");
    if (st != MFA_OK) return st;
  }
  DecodeArgs &a = args;
  set_shared_args(a, p, G, pageShift, options);
  a.R = p->rows; a.Hq = p->heads;
  a.pieces = pieces;
  if (pieces > 1) set_split_slabs(a, p->workspace, pieces, rows, set->D);
  if (quant) { a.keyScale = quant->keyScale; a.valueScale = quant->valueScale; }
  return MFA_OK;
}

hipError_t DecodePlan::run(hipStream_t stream) const {
  return run_pieces(kernel(), blocks, pieces, set->lds, set->combine, rows, stream, args);
}

// the bytes of the workspace the launch would split into: 0 for an unsplit plan, whatever workspace the caller may already have bound
mfa_status decode_workspace_size(const mfa_decode_params *params, const LaunchOptions &options, uint64_t *bytes) {
  if (bytes) *bytes = 0;
  const mfa_status refused = entry_check(options, !bytes ? "null argument" : nullptr);
  if (refused != MFA_OK) return refused;
  if (!params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_decode_params probe = *params;
  probe.workspace = nullptr;
  probe.workspaceBytes = 0;
  DecodePlan plan;
  const mfa_status st = plan.prepare(&probe, options);
  if (st != MFA_OK) return st;
  if (plan.planned > 1) *bytes = split_workspace_bytes(plan.planned, plan.rows, plan.set->D);
  return MFA_OK;
}

mfa_status decode_launch_form(const mfa_decode_params *params, const LaunchOptions &options, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  DecodePlan plan;
  mfa_status st = entry_check(options, !out || capacity == 0 ? "null argument" : nullptr);
  if (st == MFA_OK) st = plan.prepare(params, options);
  if (st != MFA_OK) return st;
  const uint32_t window = options.window;
  const Sinks &sinks = options.sinks;
  char text[512];
  const uint32_t M = plan.args.G * plan.args.R;
  // (a windowed launch names its window, its sink tokens and the tiles the piece count was chosen from; bound sink logits, then the
  // soft cap, then the tree, last)
  char cap[48] = "";
  if (options.softcap != 0.0f) std::snprintf(cap, sizeof(cap), ", softcap %g", (double)options.softcap);
  const std::string layout = std::string(plan.args.paged ? "paged" : "contiguous") +
                             (window ? ", window " + std::to_string(window) + (sinks.tokens ? ", sink tokens " + std::to_string(sinks.tokens) : "") +
                                           ": planned from " + std::to_string(plan.tiles) + " tiles"
                                     : "") +
                             (sinks.logits ? ", sink logits" : "") + cap + tree_form(options);
  if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u sequences x K/V heads x %u pieces, %u packed rows, %s) + %s (grid %llu)", plan.name(),
                  plan.blocks * plan.pieces, plan.blocks, plan.pieces, M, layout.c_str(), plan.set->combine.name,
                  (unsigned long long)combine_grid(plan.rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u sequences x K/V heads, %u packed rows, %s%s)", plan.name(), plan.blocks, M, layout.c_str(),
                  plan.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces").c_str() : "");
  copy_text(out, capacity, text);
  return MFA_OK;
}

constexpr auto decode_launch = cache_launch<DecodePlan, mfa_decode_params>;
constexpr auto decode_time = cache_time<DecodePlan, mfa_decode_params>;

} // namespace

extern "C" {

void mfa_decode_params_init(mfa_decode_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->outputPrecision = MFA_BF16;
  params->headsPerKeyValue = 1;
  params->causal = 1;
}

mfa_status mfa_attention_decode_piece_range(uint32_t length, uint32_t pieces, uint32_t piece, uint32_t *begin, uint32_t *end) {
  if (!begin || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, pieces non-zero");
  decode_piece_range(length, pieces, piece, begin, end);
  return MFA_OK;
}

mfa_status mfa_attention_decode_workspace_size(const mfa_decode_params *params, uint64_t *bytes) {
  return decode_workspace_size(params, LaunchOptions(), bytes);
}

mfa_status mfa_attention_decode_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                       void *stream) {
  return decode_launch(q, k, v, o, l, params, LaunchOptions(), stream);
}

mfa_status mfa_attention_decode_launch_form(const mfa_decode_params *params, char *out, size_t capacity) {
  return decode_launch_form(params, LaunchOptions(), out, capacity);
}

mfa_status mfa_attention_decode_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                     void *stream, int warmup, int iterations, float *milliseconds) {
  return decode_time(q, k, v, o, l, params, LaunchOptions(), stream, warmup, iterations, milliseconds);
}

// ---- over an e4m3 cache (include/mfa_kvcache.h): the same four with the cache's mfa_kv_quant, which is required

void mfa_kv_quant_init(mfa_kv_quant *quant) {
  if (!quant) return;
  std::memset(quant, 0, sizeof(*quant));
  quant->cachePrecision = MFA_KV_E4M3;
}

mfa_status mfa_attention_decode_fp8_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint64_t *bytes) {
  return decode_workspace_size(params, LaunchOptions().e4m3(quant), bytes);
}

mfa_status mfa_attention_decode_fp8_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                           const mfa_kv_quant *quant, void *stream) {
  return decode_launch(q, k, v, o, l, params, LaunchOptions().e4m3(quant), stream);
}

mfa_status mfa_attention_decode_fp8_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, char *out, size_t capacity) {
  return decode_launch_form(params, LaunchOptions().e4m3(quant), out, capacity);
}

mfa_status mfa_attention_decode_fp8_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                         const mfa_kv_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  return decode_time(q, k, v, o, l, params, LaunchOptions().e4m3(quant), stream, warmup, iterations, milliseconds);
}

// ---- under a sliding window (include/mfa_window.h): the same four with `window` after `quant`, which is null for a 16-bit cache.
// window 0 is the launch without a window, whichever cache

mfa_status mfa_attention_decode_window_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                      uint64_t *bytes) {
  return decode_workspace_size(params, LaunchOptions().cache(quant).within(window), bytes);
}

mfa_status mfa_attention_decode_window_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                              const mfa_kv_quant *quant, uint32_t window, void *stream) {
  return decode_launch(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window), stream);
}

mfa_status mfa_attention_decode_window_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window, char *out,
                                                   size_t capacity) {
  return decode_launch_form(params, LaunchOptions().cache(quant).within(window), out, capacity);
}

mfa_status mfa_attention_decode_window_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                            const mfa_kv_quant *quant, uint32_t window, void *stream, int warmup, int iterations,
                                            float *milliseconds) {
  return decode_time(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_decode_window_piece_range(uint32_t length, uint32_t rows, uint32_t window, uint32_t pieces, uint32_t piece,
                                                   uint32_t *begin, uint32_t *end) {
  if (!begin || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, pieces non-zero");
  if (window == 0 || rows == 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "window and rows must be non-zero (no window: mfa_attention_decode_piece_range)");
  decode_window_piece_range(length, rows, window, pieces, piece, begin, end);
  return MFA_OK;
}

// ---- with attention sinks (include/mfa_sink.h): the window entries with `sinks` after `window`.  The block is required; an all-zero
// one is the window launch, whichever window

void mfa_attention_sinks_init(mfa_attention_sinks *sinks) {
  if (sinks) std::memset(sinks, 0, sizeof(*sinks));
}

size_t mfa_attention_sinks_size(void) { return sizeof(mfa_attention_sinks); }

mfa_status mfa_attention_sinks_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  static const uint32_t table[] = {(uint32_t)offsetof(mfa_attention_sinks, sinkTokens), (uint32_t)offsetof(mfa_attention_sinks, reserved),
                                   (uint32_t)offsetof(mfa_attention_sinks, sinkLogits)};
  const uint32_t total = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = total;
  for (uint32_t i = 0; i < total && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_decode_sink_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                    const mfa_attention_sinks *sinks, uint64_t *bytes) {
  return decode_workspace_size(params, LaunchOptions().cache(quant).within(window).required_sinks(sinks), bytes);
}

mfa_status mfa_attention_decode_sink_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                            const mfa_kv_quant *quant, uint32_t window, const mfa_attention_sinks *sinks, void *stream) {
  return decode_launch(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window).required_sinks(sinks), stream);
}

mfa_status mfa_attention_decode_sink_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                 const mfa_attention_sinks *sinks, char *out, size_t capacity) {
  return decode_launch_form(params, LaunchOptions().cache(quant).within(window).required_sinks(sinks), out, capacity);
}

mfa_status mfa_attention_decode_sink_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                          const mfa_kv_quant *quant, uint32_t window, const mfa_attention_sinks *sinks, void *stream,
                                          int warmup, int iterations, float *milliseconds) {
  return decode_time(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window).required_sinks(sinks), stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_decode_sink_piece_range(uint32_t length, uint32_t rows, uint32_t window, uint32_t sinkTokens, uint32_t pieces,
                                                 uint32_t piece, uint32_t begin[2], uint32_t end[2]) {
  if (!begin || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, pieces non-zero");
  if (rows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "rows must be non-zero");
  if (sinkTokens && !window) return fail(MFA_ERR_INVALID_ARGUMENT, "sink tokens need a window: sinkTokens must be 0 when window is 0");
  decode_sink_piece_range(length, rows, window, sinkTokens, pieces, piece, begin, end);
  return MFA_OK;
}

// ---- with a soft cap (include/mfa_softcap.h): the sink entries with `softcap` after `sinks`, which may be NULL here (no sinks).
// softcap 0 is the launch of the headers below, whichever window and sinks

mfa_status mfa_attention_decode_softcap_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                       const mfa_attention_sinks *sinks, float softcap, uint64_t *bytes) {
  return decode_workspace_size(params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).capped(softcap), bytes);
}

mfa_status mfa_attention_decode_softcap_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                               const mfa_kv_quant *quant, uint32_t window, const mfa_attention_sinks *sinks, float softcap,
                                               void *stream) {
  return decode_launch(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).capped(softcap), stream);
}

mfa_status mfa_attention_decode_softcap_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                    const mfa_attention_sinks *sinks, float softcap, char *out, size_t capacity) {
  return decode_launch_form(params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).capped(softcap), out, capacity);
}

mfa_status mfa_attention_decode_softcap_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                             const mfa_kv_quant *quant, uint32_t window, const mfa_attention_sinks *sinks, float softcap,
                                             void *stream, int warmup, int iterations, float *milliseconds) {
  return decode_time(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).capped(softcap), stream, warmup, iterations, milliseconds);
}

// ---- with a speculation tree (include/mfa_tree.h): the sink entries with `tree` after `sinks`, which may be NULL here (no sinks).  The
// tree block is required

void mfa_attention_tree_init(mfa_attention_tree *tree) {
  if (tree) std::memset(tree, 0, sizeof(*tree));
}

size_t mfa_attention_tree_size(void) { return sizeof(mfa_attention_tree); }

mfa_status mfa_attention_tree_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  static const uint32_t table[] = {(uint32_t)offsetof(mfa_attention_tree, masks), (uint32_t)offsetof(mfa_attention_tree, batchStride),
                                   (uint32_t)offsetof(mfa_attention_tree, reserved)};
  *count = 3;
  for (uint32_t i = 0; i < 3 && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_decode_tree_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                    const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, uint64_t *bytes) {
  return decode_workspace_size(params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).tree_of(tree), bytes);
}

mfa_status mfa_attention_decode_tree_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                            const mfa_kv_quant *quant, uint32_t window, const mfa_attention_sinks *sinks,
                                            const mfa_attention_tree *tree, void *stream) {
  return decode_launch(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).tree_of(tree), stream);
}

mfa_status mfa_attention_decode_tree_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, uint32_t window,
                                                 const mfa_attention_sinks *sinks, const mfa_attention_tree *tree, char *out, size_t capacity) {
  return decode_launch_form(params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).tree_of(tree), out, capacity);
}

mfa_status mfa_attention_decode_tree_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                          const mfa_kv_quant *quant, uint32_t window, const mfa_attention_sinks *sinks,
                                          const mfa_attention_tree *tree, void *stream, int warmup, int iterations, float *milliseconds) {
  return decode_time(q, k, v, o, l, params, LaunchOptions().cache(quant).within(window).optional_sinks(sinks).tree_of(tree), stream, warmup, iterations, milliseconds);
}

} // extern "C"
