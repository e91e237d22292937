// cache_launch.h -- what the host sides of the launches over a KV cache share (attn_decode16.hip, attn_prefill16.hip,
// kv_cache_append.hip, kv_cache_compact.hip): the checks of paging, operand strides, cache precision and buffer pointers, and of a sliding window and
// attention sinks (Sinks, check_window_and_sinks: decode and prefill), of a soft cap (check_softcap) and of a speculation tree
// (check_tree), each with ONE wording, so that the same mistake is refused in the same words whichever launch meets it; the options of a launch as one value (LaunchOptions), and the
// path every decode and prefill entry takes from it: the checks both launches word alike (check_precisions ... check_cache_and_strides), bind, the
// launch cut along the keys (choose_pieces ... run_pieces: the piece count, the workspace and its check, the slabs, the two kernels of a
// run) and the bodies of the launch and time entries (cache_launch, cache_time).  hip_fail, copy_text and time_launches also serve mfa_kernel.hip.
// Internal, not part of the ABI.  Every check records its message (fail, mfa_internal.h) and returns the status.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>

#include "../../include/mfa_kvcache.h"
#include "../../include/mfa_ragged.h"
#include "../../include/mfa_sink.h"
#include "../../include/mfa_split.h"
#include "../../include/mfa_tree.h"
#include "launchers.h"
#include "mfa_internal.h"

namespace mfa {

// MFA_ERR_HIP, "<what>: <error name> (<error string>)"
mfa_status hip_fail(hipError_t err, const char *what);

// a launch form's text into the caller's buffer (capacity > 0), cut to fit, always terminated
void copy_text(char *out, size_t capacity, const char *text);

// pageSize 0 is a contiguous cache (*pageShift = 0); otherwise a power of two from 16 to 1024 with a block table, *pageShift its
// logarithm.  `column` != 0: a sequence's row of the table must hold the pages of that many keys (decode, prefill).  0: any positive
// stride (append, whose kernel drops a row whose page lies past the stride).
mfa_status check_paging(uint32_t pageSize, const void *blockTable, int64_t blockTableStride, uint32_t column, uint32_t *pageShift);

// the cache of a launch that WRITES it (append, compact): check_paging without a column bound -- the kernels drop a row whose page lies
// past the stride (kv_cache_slot.h) -- and, for a contiguous cache, a non-zero `column`
mfa_status check_written_cache(uint32_t pageSize, const void *blockTable, int64_t blockTableStride, uint32_t column, uint32_t *pageShift);
// ... and the strides of its kCache / vCache (`name`), in check_operand_strides' words: multiples of 8 elements, an e4m3 cache of 16
mfa_status check_written_cache_strides(const char *name, uint32_t headDimension, int64_t leadingDimension, int64_t headStride, int64_t outer, bool fp8);
extern const char *const kWrittenCacheStridesWhy;

// one operand's strides, in elements: leadingDimension, headStride and `outer` (the batch stride, or the page stride of a paged cache)
// are multiples of `need`; `why` ends the message.  check_operand_strides first wants rows of at least headDimension elements.
mfa_status check_stride_multiples(const char *name, int64_t leadingDimension, int64_t headStride, int64_t outer, int64_t need, const char *why);
mfa_status check_operand_strides(const char *name, uint32_t headDimension, int64_t leadingDimension, int64_t headStride, int64_t outer,
                                 int64_t need, const char *why);

// MFA_KV_E5M2 is refused; *fp8 = the cache is MFA_KV_E4M3.  (What else a launch takes, and its words for it, stay with the launch.)
mfa_status check_cache_precision(uint32_t cachePrecision, bool *fp8);

// buffers a kernel reads or writes 16 bytes at a time: all non-null, all 16-byte aligned; `names` as the message lists them
mfa_status check_buffers(std::initializer_list<const void *> buffers, const char *names);
// optional FP32 arrays: null or 4-byte aligned
mfa_status check_float_arrays(std::initializer_list<const void *> arrays, const char *names);

// the sinks of a launch (include/mfa_sink.h): none for the entries of the other headers
struct Sinks {
  uint32_t tokens = 0;
  const float *logits = nullptr;
  bool any() const { return tokens != 0 || logits != nullptr; }
};
// sink tokens need a window and causal; a window (0: none) needs causal
mfa_status check_window_and_sinks(uint32_t window, const Sinks &sinks, bool causal);
// the soft cap of a launch (include/mfa_softcap.h): 0 is none, anything but a finite positive number is refused
mfa_status check_softcap(float softcap);
// The 64-key tiles a sequence can walk, from what the host knows (the lengths live on the device): what decode's piece count and the
// split prefill launch's are chosen from.  Under a window of W keys a sequence walks the tiles of W + rows - 1 keys that need not start
// on a tile: at most ceil((W + rows - 1) / 64) + 1, and never more than column's.  S sink tokens add at most their ceil(S / 64) tiles
// to the window's.
inline uint64_t planned_tiles(uint32_t column, uint32_t rows, uint32_t window, uint32_t sinkTokens) {
  const uint64_t tiles = ((uint64_t)column + MFA_DECODE_KEY_TILE - 1) / MFA_DECODE_KEY_TILE;
  if (!window) return tiles;
  const uint64_t spanned = ((uint64_t)window + rows - 1 + MFA_DECODE_KEY_TILE - 1) / MFA_DECODE_KEY_TILE + 1 +
                           ((uint64_t)sinkTokens + MFA_DECODE_KEY_TILE - 1) / MFA_DECODE_KEY_TILE;
  return spanned < tiles ? spanned : tiles;
}
struct LaunchOptions;
// the tree of a launch (include/mfa_tree.h; none: MFA_OK): it needs causal, a window of 0 or at least `rows` keys, at most `rowLimit`
// rows (0: the launch has its own limit), masks that are bound and 8-byte aligned, and neither a soft cap nor packed rows -- in this order
mfa_status check_tree(const LaunchOptions &options, bool causal, uint32_t rows, uint32_t rowLimit);
// ", tree masks" and how they are shared, for a launch form; empty without a tree
std::string tree_form(const LaunchOptions &options);

// The options of a launch beside its params: what the entry families of mfa_kvcache.h (fp8_), mfa_window.h, mfa_sink.h, mfa_ragged.h,
// mfa_softcap.h and mfa_tree.h add to the plain entries, as ONE value that every function below an entry takes.  An entry builds it in one statement
// from the setters, each of which carries its argument's NULL rule in that family's words; a new option is a member, a setter and the
// places that read it.
struct LaunchOptions {
  const mfa_kv_quant *quant = nullptr;       // decode over an e4m3 cache (prefill says it in its params); null: a 16-bit cache
  uint32_t window = 0;                       // 0: none
  Sinks sinks;
  const mfa_ragged_rows *ragged = nullptr;   // prefill over packed rows; null: padded
  float softcap = 0.0f;                      // 0: none
  const mfa_attention_tree *tree = nullptr;  // a speculation tree among the new rows; null: the causal rule
  const mfa_key_split *split = nullptr;      // prefill cut along the keys (include/mfa_split.h); null: the launch of the other headers
  const char *refusal = nullptr;             // a block the family requires is NULL: what entry_check answers
  bool refusalFirst = true;                  // ... before the entry's own arguments are looked at (fp8_: after)

  LaunchOptions &e4m3(const mfa_kv_quant *block);                  // the fp8_ entries: required
  LaunchOptions &cache(const mfa_kv_quant *block) { quant = block; return *this; }   // the later decode entries: NULL is a 16-bit cache
  LaunchOptions &within(uint32_t keys) { window = keys; return *this; }
  LaunchOptions &required_sinks(const mfa_attention_sinks *block);   // the sink_ entries
  LaunchOptions &optional_sinks(const mfa_attention_sinks *block);   // the ragged_ and softcap_ entries: NULL is no sinks
  LaunchOptions &ragged_of(const mfa_ragged_rows *block);            // the ragged_ entries: required
  LaunchOptions &capped(float cap) { softcap = cap; return *this; }
  LaunchOptions &tree_of(const mfa_attention_tree *block);           // the tree_ entries: required
  LaunchOptions &optional_tree(const mfa_attention_tree *block) { tree = block; return *this; }   // the split_ entries: NULL is no tree
  LaunchOptions &split_of(const mfa_key_split *block);               // the split_ entries: required
};
// what an entry answers before its launch is prepared: the options' refusal and `bad`, what is wrong with the entry's own arguments
// (null: nothing), in the family's order
mfa_status entry_check(const LaunchOptions &options, const char *bad);

// The checks mfa_decode_params and mfa_prefill_params are put to in the same words.  Each prepare calls them in this order, with its own
// checks (its kernel table, prefill's cache precision, the limits of its packing) between them where they have always stood: the order
// in which two mistakes are reported is pinned by tests/golden/cache_refusals.json.
mfa_status check_precisions(int precision, int outputPrecision);
template <typename Params>
mfa_status check_sizes(const Params *p) {
  if (p->rows == 0 || p->column == 0 || p->heads == 0 || p->batches == 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "rows, column, heads and batches must be non-zero");
  return MFA_OK;
}
mfa_status check_group(uint32_t heads, uint32_t G);
// cacheLengths, the paging (*pageShift: out) and the strides of Q, K, V and O; `e4m3Rows`: K and V rows of bytes, strides in multiples of 16
template <typename Params>
mfa_status check_cache_and_strides(const Params *p, bool e4m3Rows, uint32_t *pageShift) {
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  mfa_status st = check_paging(p->pageSize, p->blockTable, p->blockTableStride, p->column, pageShift);
  if (st != MFA_OK) return st;
  static const char *names[4] = {"Q", "K", "V", "O"};
  for (int i = 0; i < 4; ++i) {
    const bool kv = i == 1 || i == 2;
    const int64_t need = (i == 3) ? 4 : (kv && e4m3Rows) ? 16 : 8;   // 16-byte rows of Q, K, V; 8- or 16-byte stores of O
    st = check_operand_strides(names[i], p->headDimension, p->leadingDimension[i], p->headStride[i],
                               kv && p->pageSize ? p->pageStride[i - 1] : p->batchStride[i], need,
                               kv && e4m3Rows ? "(16-byte rows of an e4m3 cache)" : "(16-byte rows for Q, K, V; whole 4-element stores for O)");
    if (st != MFA_OK) return st;
  }
  return MFA_OK;
}

// what DecodeArgs and PrefillArgs (attn_decode16.h, attn_prefill16.h) share, from the params and options of a checked launch; the rest
// of the block is zero
template <typename Args, typename Params>
void set_shared_args(Args &a, const Params *p, uint32_t G, uint32_t pageShift, const LaunchOptions &options) {
  std::memset(&a, 0, sizeof(a));
  a.lengths = p->cacheLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.hsk = p->headStride[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride[0];
  a.ldv = p->leadingDimension[2]; a.hsv = p->headStride[2]; a.bsv = p->batchStride[2]; a.psv = p->pageStride[1];
  a.ldo = p->leadingDimension[3]; a.hso = p->headStride[3]; a.bso = p->batchStride[3];
  a.lhs = p->lHeadStride; a.lbs = p->lBatchStride;
  a.G = G; a.Hkv = p->heads / G; a.batches = p->batches; a.column = p->column;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0; a.outF32 = p->outputPrecision == MFA_FP32;
  a.scale2 = 1.44269504089f / std::sqrt((float)p->headDimension);
  a.window = options.window;
  a.sinkTokens = options.sinks.tokens;
  a.sinkLogits = options.sinks.logits;
  if (options.softcap != 0.0f) {   // cap x tanh(s / cap) in the kernels' log2 units
    a.capIn = 2.0f / options.softcap;
    a.capOut = options.softcap * 1.44269504089f;
  }
  if (options.tree) {
    a.masks = options.tree->masks;
    a.maskStride = options.tree->batchStride;
  }
}

// the buffers of a launch into a plan's argument block
template <typename Plan>
mfa_status bind(Plan *plan, const void *q, const void *k, const void *v, void *o, float *l) {
  mfa_status st = check_buffers({q, k, v, o}, "Q, K, V and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st == MFA_OK) st = check_float_arrays({plan->args.keyScale, plan->args.valueScale}, "keyScale and valueScale");
  if (st == MFA_OK) st = check_float_arrays({plan->args.sinkLogits}, "sinkLogits");
  if (st != MFA_OK) return st;
  plan->args.q = (const char *)q; plan->args.k = (const char *)k; plan->args.v = (const char *)v;
  plan->args.o = (char *)o; plan->args.l = l;
  return MFA_OK;
}

// ---- The launch cut along the keys, as DecodePlan and PrefillPlan (include/mfa_split.h) run it: every block's keys go to `pieces`
// workgroups that publish un-normalised O and (m, l) in FP32 to the caller's workspace -- wsO [pieces][rows][D], then wsML
// [pieces][rows][2], rows = batches x query heads x rows -- and a combine kernel, one wave per row, merges them.

// a kernel of a plan's table: the function and its name, which a launch form and a HIP failure are reported under
template <typename Args> struct CacheKernel {
  void (*launch)(const Args);
  const char *name;
};
#define MFA_CACHE_KERNEL(NAME) {NAME, #NAME}

// The piece count, from the workgroups the launch has without a split and planned_tiles only -- the lengths live on the device.  Aims
// at `target` workgroups, rounded down; a piece keeps at least `minTiles` tiles; at most `maxPieces`; below 2: 1.
uint32_t choose_pieces(uint64_t blocks, uint64_t tiles, uint64_t target, uint64_t minTiles, uint64_t maxPieces);
// the project's one workspace formula, in bytes
inline uint64_t split_workspace_bytes(uint32_t pieces, uint64_t rows, uint32_t D) { return (uint64_t)pieces * rows * (D + 2) * sizeof(float); }
// the workspace of a launch in more than one piece: at least `need` bytes -- `sizeEntry` is the entry that says how many -- and 16-byte aligned
mfa_status check_split_workspace(const void *workspace, uint64_t bytes, uint64_t need, const char *sizeEntry);
template <typename Args> void set_split_slabs(Args &a, void *workspace, uint32_t pieces, uint64_t rows, uint32_t D) {
  a.pieces = pieces;
  a.wsO = (float *)workspace;
  a.wsML = a.wsO + (uint64_t)pieces * rows * D;
}
inline uint64_t combine_grid(uint64_t rows) { return (rows + 3) / 4; }   // a wave per row, four to a workgroup
// the body of a plan's run(): the kernel that reads the cache on blocks x pieces workgroups, then -- more than one piece -- the combine
// kernel over the slabs' `rows`, both on the caller's stream; nothing synchronises
template <typename Args>
hipError_t run_pieces(const CacheKernel<Args> &kernel, uint32_t blocks, uint32_t pieces, uint32_t lds, const CacheKernel<Args> &combine,
                      uint64_t rows, hipStream_t stream, const Args &args) {
  hipError_t err = launch_kernel(kernel.launch, dim3(blocks * pieces), dim3(256), lds, stream, args);
  if (err == hipSuccess && pieces > 1) err = launch_kernel(combine.launch, dim3((uint32_t)combine_grid(rows)), dim3(256), 0, stream, args);
  return err != hipSuccess ? err : hipGetLastError();
}

// Times `iterations` calls of run(stream) between two events, after `warmup` untimed ones; nothing more is started after a call that
// failed.  `name` is the kernel a HIP failure is reported under.
template <typename Run>
mfa_status time_launches(hipStream_t stream, int warmup, int iterations, float *milliseconds, const char *name, Run run) {
  hipEvent_t start, stop;
  hipError_t err = hipEventCreate(&start);
  if (err != hipSuccess) return hip_fail(err, "hipEventCreate");
  err = hipEventCreate(&stop);
  if (err != hipSuccess) { (void)hipEventDestroy(start); return hip_fail(err, "hipEventCreate"); }
  for (int i = 0; i < warmup && err == hipSuccess; ++i) err = run(stream);
  if (err == hipSuccess) err = hipEventRecord(start, stream);
  for (int i = 0; i < iterations && err == hipSuccess; ++i) err = run(stream);
  if (err == hipSuccess) err = hipEventRecord(stop, stream);
  if (err == hipSuccess) err = hipEventSynchronize(stop);
  if (err == hipSuccess) err = hipGetLastError();
  if (err == hipSuccess) err = hipEventElapsedTime(milliseconds, start, stop);
  (void)hipEventDestroy(start);
  (void)hipEventDestroy(stop);
  if (err != hipSuccess) return hip_fail(err, name);
  return MFA_OK;
}

// The bodies of every decode and prefill `_launch` and `_time` entry.  Plan: DecodePlan / PrefillPlan, with prepare(params, options),
// run(stream) and name() -- the kernel a HIP failure is reported under.
template <typename Plan, typename Params>
mfa_status cache_launch(const void *q, const void *k, const void *v, void *o, float *l, const Params *params, const LaunchOptions &options,
                        void *stream) {
  Plan plan;
  mfa_status st = entry_check(options, nullptr);
  if (st == MFA_OK) st = plan.prepare(params, options);
  if (st == MFA_OK) st = bind(&plan, q, k, v, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

template <typename Plan, typename Params>
mfa_status cache_time(const void *q, const void *k, const void *v, void *o, float *l, const Params *params, const LaunchOptions &options,
                      void *stream, int warmup, int iterations, float *milliseconds) {
  Plan plan;
  mfa_status st = entry_check(options, !milliseconds || iterations <= 0 || warmup < 0 ? "bad timing arguments" : nullptr);
  if (st == MFA_OK) st = plan.prepare(params, options);
  if (st == MFA_OK) st = bind(&plan, q, k, v, o, l);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

} // namespace mfa
