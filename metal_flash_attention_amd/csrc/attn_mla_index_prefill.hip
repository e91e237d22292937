// attn_mla_index_prefill.hip -- the prefill indexer: the kernels' code objects (attn_mla_index_prefill.h) and the C ABI of
// include/mfa_mla_index_prefill.h -- the index logits of a prompt chunk of any number of rows, the top-k selection under prefill's
// frontier, and their chain in passes of rows.  A translation unit of its own.  Every check of mfa_mla_index_params is
// mla_index_checks.h's, in the decode indexer's order and words and without its rows limit; what this unit adds is the span plan of the
// logits launch, the pass plan of the chain and its workspace.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN where nothing is visible.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_index_prefill.h"
#include "attn_mla_index_prefill.h"
#include "launchers.h"
#include "mla_index_checks.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace.
extern "C" __global__ __launch_bounds__(256) void attn_mlaip_d128_bf16(const mfa::MlaIndexPrefillArgs a) {
  mfa::mla_index_prefill_logits_body<__bf16>(a);
}
extern "C" __global__ __launch_bounds__(256) void attn_mlaip_d128_f16(const mfa::MlaIndexPrefillArgs a) {
  mfa::mla_index_prefill_logits_body<_Float16>(a);
}
extern "C" __global__ __launch_bounds__(1024) void attn_mlaip_select(const mfa::MlaIndexPrefillArgs a) {
  mfa::mla_index_select_body<mfa::MlaipRule>(a);
}

namespace {

typedef CacheKernel<MlaIndexPrefillArgs> PrefillIndexKernel;
const PrefillIndexKernel kLogits[2] = {MFA_CACHE_KERNEL(attn_mlaip_d128_bf16), MFA_CACHE_KERNEL(attn_mlaip_d128_f16)};
const PrefillIndexKernel kSelect = MFA_CACHE_KERNEL(attn_mlaip_select);

static_assert(MLAIP_TILE == MFA_MLA_INDEX_PREFILL_TILE, "the header states the kernel's tile");
constexpr uint64_t kWorkgroupTarget = 512;                         // 256 compute units x two workgroups: rows are cut into spans up to here
constexpr uint64_t kMinSpan = MFA_MLA_INDEX_PREFILL_MIN_SPAN;      // ... but a span keeps the 64 KiB key load amortised against 16 KiB a row
constexpr uint64_t kMaxSpan = MFA_MLA_INDEX_PREFILL_MAX_SPAN;      // ... and stays short enough for a pass of the chain to be a few of them

struct PrefillIndexPlan {
  MlaIndexPrefillArgs args;    // of the first pass; run() moves row0 / R / spans and the lists' rows along
  const PrefillIndexKernel *logits;
  int stage;
  uint32_t tiles, span;
  uint32_t passRows, passes;   // rows of a pass (all of them outside the chain), passes of the chunk
  mfa_status prepare(const mfa_mla_index_params *p, const uint32_t *queryLengths, int stage);
  const char *name() const { return stage & MLAI_LOGITS ? logits->name : kSelect.name; }
  uint32_t spans_of(uint32_t rows) const { return (rows + span - 1) / span; }
  hipError_t run(hipStream_t stream) const {
    hipError_t err = hipSuccess;
    MlaIndexPrefillArgs a = args;
    for (uint32_t pass = 0; pass < passes && err == hipSuccess; ++pass) {
      a.row0 = pass * passRows;
      a.R = std::min(passRows, a.rowsAll - a.row0);
      a.spans = spans_of(a.R);
      if (stage & MLAI_LOGITS) err = launch_kernel(logits->launch, dim3(tiles * a.spans * a.batches), dim3(256), 0, stream, a);
      if (err == hipSuccess && (stage & MLAI_SELECT))
        err = launch_kernel(kSelect.launch, dim3(a.R * a.batches), dim3(MLAI_SELECT_THREADS), 0, stream, a);
    }
    return err != hipSuccess ? err : hipGetLastError();
  }
};

// every check that needs no GPU, and the kernels' argument block (the buffer pointers are filled in by the entries)
mfa_status PrefillIndexPlan::prepare(const mfa_mla_index_params *p, const uint32_t *queryLengths, int which) {
  mfa_status st = check_index_block(p, 0);
  if (st != MFA_OK) return st;
  stage = which;
  uint32_t pageShift = 0;
  logits = nullptr;
  // the spans: as many as bring the grid to kWorkgroupTarget, of whole multiples of kMinSpan rows, at most kMaxSpan
  const uint64_t tiles64 = ((uint64_t)p->column + MLAIP_TILE - 1) / MLAIP_TILE;
  const uint64_t wanted = (kWorkgroupTarget + tiles64 * p->batches - 1) / (tiles64 * p->batches);
  const uint64_t span64 = std::min((std::max<uint64_t>((p->rows + wanted - 1) / wanted, 1) + kMinSpan - 1) / kMinSpan * kMinSpan, kMaxSpan);
  const uint64_t spans64 = (p->rows + span64 - 1) / span64;
  if (stage & MLAI_LOGITS) {
    if ((st = check_index_logits(p, &pageShift)) != MFA_OK) return st;
    if (tiles64 * spans64 * p->batches > 0x7FFFFFFFull)
      return fail(MFA_ERR_INVALID_ARGUMENT, "tiles x spans x batches must fit a grid of 2^31 - 1 workgroups");
  }
  if ((stage & MLAI_SELECT) && (st = check_index_select(p)) != MFA_OK) return st;
  int64_t lrs = p->logitRowStride, lbs = p->logitBatchStride;
  uint64_t rowsOfPass = p->rows;
  if (stage == MLAI_TOPK) {   // the logits of a pass live in the workspace, packed
    lrs = (int64_t)mlai_padded_column(p->column);
    const uint64_t rowBytes = (uint64_t)p->batches * lrs * sizeof(float);   // one row of every sequence
    if (!p->workspace)
      return fail(MFA_ERR_INVALID_ARGUMENT, "workspace is required: mfa_mla_index_prefill_topk_launch keeps the logits of a pass of rows in it, at least " +
                                                std::to_string(rowBytes * std::min<uint64_t>(span64, p->rows)) +
                                                " bytes (mfa_mla_index_prefill_workspace_size)");
    rowsOfPass = p->workspaceBytes / rowBytes;
    if (rowsOfPass < p->rows) rowsOfPass = rowsOfPass / span64 * span64;   // whole spans, unless the chunk fits
    if (rowsOfPass == 0)
      return fail(MFA_ERR_INVALID_ARGUMENT, "workspace too small: workspaceBytes = " + std::to_string(p->workspaceBytes) +
                                                ", a pass needs one span of " + std::to_string(std::min<uint64_t>(span64, p->rows)) +
                                                " rows per sequence, " + std::to_string(rowBytes * std::min<uint64_t>(span64, p->rows)) +
                                                " bytes (mfa_mla_index_prefill_workspace_size)");
    rowsOfPass = std::min<uint64_t>(rowsOfPass, p->rows);
    if ((uintptr_t)p->workspace % 16 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    lbs = lrs * (int64_t)rowsOfPass;
  } else if ((st = check_index_logit_stride(p)) != MFA_OK) {
    return st;
  }
  tiles = (uint32_t)tiles64;
  span = (uint32_t)span64;
  passRows = (uint32_t)rowsOfPass;
  passes = (uint32_t)((p->rows + rowsOfPass - 1) / rowsOfPass);
  MlaIndexPrefillArgs &a = args;
  std::memset(&a, 0, sizeof(a));
  fill_index_args(a, p, pageShift);
  a.lrs = lrs; a.lbs = lbs;
  a.tiles = tiles;
  a.qlengths = queryLengths;
  a.rowsAll = p->rows;
  a.span = span;
  a.R = passRows;
  a.spans = spans_of(passRows);
  if (stage & MLAI_LOGITS) logits = &kLogits[p->precision == MFA_FP16];
  if (stage == MLAI_TOPK) a.logits = (float *)p->workspace;
  return MFA_OK;
}

mfa_status prefill_index_launch(int stage, const void *qi, const float *w, const void *ki, float *logits, int32_t *indices,
                                const mfa_mla_index_params *params, const uint32_t *queryLengths, void *stream) {
  PrefillIndexPlan plan;
  mfa_status st = plan.prepare(params, queryLengths, stage);
  if (st == MFA_OK) st = bind_index(plan.args, stage, qi, w, ki, logits, indices);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status prefill_index_time(int stage, const void *qi, const float *w, const void *ki, float *logits, int32_t *indices,
                              const mfa_mla_index_params *params, const uint32_t *queryLengths, void *stream, int warmup, int iterations,
                              float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  PrefillIndexPlan plan;
  mfa_status st = plan.prepare(params, queryLengths, stage);
  if (st == MFA_OK) st = bind_index(plan.args, stage, qi, w, ki, logits, indices);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

mfa_status prefill_index_launch_form(int stage, const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  PrefillIndexPlan plan;
  const mfa_status st = plan.prepare(params, queryLengths, stage);
  if (st != MFA_OK) return st;
  const MlaIndexPrefillArgs &a = plan.args;   // the first pass: the largest
  char first[256] = "", second[128] = "", third[64] = "";
  if (stage & MLAI_LOGITS)
    std::snprintf(first, sizeof(first), "%s (grid %u = %u tiles of %u keys x %u spans of %u rows x %u sequences, %u heads, %s)", plan.logits->name,
                  plan.tiles * a.spans * a.batches, plan.tiles, (unsigned)MLAIP_TILE, a.spans, plan.span, a.batches, a.H, a.paged ? "paged" : "contiguous");
  if (stage & MLAI_SELECT)
    std::snprintf(second, sizeof(second), "%s (grid %u = %u rows x %u sequences, topk %u)", kSelect.name, a.R * a.batches, a.R, a.batches, a.topk);
  if (stage == MLAI_TOPK) std::snprintf(third, sizeof(third), ", %u passes of %u rows", plan.passes, plan.passRows);
  const std::string text = std::string(first) + (stage == MLAI_TOPK ? " + " : "") + second + third;
  copy_text(out, capacity, text.c_str());
  return MFA_OK;
}

} // namespace

extern "C" {

mfa_status mfa_mla_index_prefill_workspace_size(const mfa_mla_index_params *params, const uint32_t *queryLengths, uint64_t *bytes) {
  if (bytes) *bytes = 0;
  if (!bytes || !params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_mla_index_params probe = *params;   // every check of the chain but the workspace's own
  static float aligned[4] __attribute__((aligned(16)));
  probe.workspace = aligned;
  probe.workspaceBytes = ~0ull;
  PrefillIndexPlan plan;
  const mfa_status st = plan.prepare(&probe, queryLengths, MLAI_TOPK);
  if (st != MFA_OK) return st;
  // the whole chunk, or what the cap holds in whole spans -- never less than one span per sequence
  const uint64_t rowBytes = (uint64_t)params->batches * mlai_padded_column(params->column) * sizeof(float);
  const uint64_t capRows = std::max<uint64_t>(MFA_MLA_INDEX_PREFILL_WORKSPACE_CAP / rowBytes / plan.span, 1) * plan.span;
  *bytes = rowBytes * std::min<uint64_t>(params->rows, capRows);
  return MFA_OK;
}

mfa_status mfa_mla_index_prefill_logits_launch(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                               const uint32_t *queryLengths, void *stream) {
  return prefill_index_launch(MLAI_LOGITS, qi, w, ki, logits, nullptr, params, queryLengths, stream);
}
mfa_status mfa_mla_index_prefill_logits_launch_form(const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity) {
  return prefill_index_launch_form(MLAI_LOGITS, params, queryLengths, out, capacity);
}
mfa_status mfa_mla_index_prefill_logits_time(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                             const uint32_t *queryLengths, void *stream, int warmup, int iterations, float *milliseconds) {
  return prefill_index_time(MLAI_LOGITS, qi, w, ki, logits, nullptr, params, queryLengths, stream, warmup, iterations, milliseconds);
}

mfa_status mfa_mla_index_prefill_select_launch(const float *logits, int32_t *indices, const mfa_mla_index_params *params,
                                               const uint32_t *queryLengths, void *stream) {
  return prefill_index_launch(MLAI_SELECT, nullptr, nullptr, nullptr, const_cast<float *>(logits), indices, params, queryLengths, stream);
}
mfa_status mfa_mla_index_prefill_select_launch_form(const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity) {
  return prefill_index_launch_form(MLAI_SELECT, params, queryLengths, out, capacity);
}
mfa_status mfa_mla_index_prefill_select_time(const float *logits, int32_t *indices, const mfa_mla_index_params *params, const uint32_t *queryLengths,
                                             void *stream, int warmup, int iterations, float *milliseconds) {
  return prefill_index_time(MLAI_SELECT, nullptr, nullptr, nullptr, const_cast<float *>(logits), indices, params, queryLengths, stream, warmup,
                            iterations, milliseconds);
}

mfa_status mfa_mla_index_prefill_topk_launch(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                             const uint32_t *queryLengths, void *stream) {
  return prefill_index_launch(MLAI_TOPK, qi, w, ki, nullptr, indices, params, queryLengths, stream);
}
mfa_status mfa_mla_index_prefill_topk_launch_form(const mfa_mla_index_params *params, const uint32_t *queryLengths, char *out, size_t capacity) {
  return prefill_index_launch_form(MLAI_TOPK, params, queryLengths, out, capacity);
}
mfa_status mfa_mla_index_prefill_topk_time(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                           const uint32_t *queryLengths, void *stream, int warmup, int iterations, float *milliseconds) {
  return prefill_index_time(MLAI_TOPK, qi, w, ki, nullptr, indices, params, queryLengths, stream, warmup, iterations, milliseconds);
}

} // extern "C"
