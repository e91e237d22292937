// attn_mla_index.hip -- the MLA sparse indexer: the kernels' code objects (attn_mla_index.h) and the C ABI of include/mfa_mla_index.h --
// the index logits, the top-k selection and their chain.  A translation unit of its own.  The checks of the cache's paging and of the
// operands' strides are cache_launch.h's, in its words; the checks of the block's own fields are mla_index_checks.h's, shared with the
// prefill indexer; what this unit adds is its rows limit, the tile plan of the logits launch and its workspace.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN where nothing is visible.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "launchers.h"
#include "mla_index_checks.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace.
extern "C" __global__ __launch_bounds__(256) void attn_mlai_d128_bf16(const mfa::MlaIndexArgs a) { mfa::mla_index_logits_body<__bf16>(a); }
extern "C" __global__ __launch_bounds__(256) void attn_mlai_d128_f16(const mfa::MlaIndexArgs a) { mfa::mla_index_logits_body<_Float16>(a); }
extern "C" __global__ __launch_bounds__(1024) void attn_mlai_select(const mfa::MlaIndexArgs a) { mfa::mla_index_select_body<mfa::MlaiDecodeRule>(a); }

namespace {

typedef CacheKernel<MlaIndexArgs> IndexKernel;
const IndexKernel kLogits[2] = {MFA_CACHE_KERNEL(attn_mlai_d128_bf16), MFA_CACHE_KERNEL(attn_mlai_d128_f16)};
const IndexKernel kSelect = MFA_CACHE_KERNEL(attn_mlai_select);

constexpr uint32_t kTileKeys = MFA_MLA_INDEX_KEY_STEP * MLAI_WAVES;   // keys of a workgroup's step
constexpr uint64_t kWorkgroupTarget = 1024;                           // a tile grows while the grid keeps this many workgroups
constexpr uint32_t kMaxSteps = 8;

enum Stage { LOGITS = MLAI_LOGITS, SELECT = MLAI_SELECT, TOPK = MLAI_TOPK };

inline uint64_t padded_column(uint32_t column) { return mlai_padded_column(column); }
inline uint64_t workspace_bytes(const mfa_mla_index_params *p) { return (uint64_t)p->batches * p->rows * padded_column(p->column) * sizeof(float); }

struct IndexPlan {
  MlaIndexArgs args;
  const IndexKernel *logits;
  int stage;
  uint32_t grid;         // of the logits kernel: tiles x rows x batches
  uint32_t lists;        // of the select kernel: rows x batches
  mfa_status prepare(const mfa_mla_index_params *p, int stage);
  const char *name() const { return stage & LOGITS ? logits->name : kSelect.name; }
  hipError_t run(hipStream_t stream) const {
    hipError_t err = hipSuccess;
    if (stage & LOGITS) err = launch_kernel(logits->launch, dim3(grid), dim3(256), 0, stream, args);
    if (err == hipSuccess && (stage & SELECT)) err = launch_kernel(kSelect.launch, dim3(lists), dim3(MLAI_SELECT_THREADS), 0, stream, args);
    return err != hipSuccess ? err : hipGetLastError();
  }
};

// every check that needs no GPU, and the kernels' argument block (the buffer pointers are filled in by the entries)
mfa_status IndexPlan::prepare(const mfa_mla_index_params *p, int which) {
  mfa_status st = check_index_block(p, MFA_MLA_PACKED_ROWS);
  if (st != MFA_OK) return st;
  stage = which;
  const uint64_t lists64 = (uint64_t)p->rows * p->batches;
  uint32_t pageShift = 0;
  uint64_t tiles = 1, steps = 1;
  logits = nullptr;
  if (stage & LOGITS) {
    if ((st = check_index_logits(p, &pageShift)) != MFA_OK) return st;
    // the tile: a wave walks `steps` steps, doubled while the grid keeps kWorkgroupTarget workgroups
    const uint64_t steps128 = ((uint64_t)p->column + kTileKeys - 1) / kTileKeys;
    while (steps < kMaxSteps && (steps128 / (2 * steps)) * lists64 >= kWorkgroupTarget) steps *= 2;
    tiles = (steps128 + steps - 1) / steps;
    if (tiles * lists64 > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "tiles x rows x batches must fit a grid of 2^31 - 1 workgroups");
  }
  if ((stage & SELECT) && (st = check_index_select(p)) != MFA_OK) return st;
  int64_t lrs = p->logitRowStride, lbs = p->logitBatchStride;
  if (stage == TOPK) {   // the logits live in the workspace, packed
    const uint64_t need = workspace_bytes(p);
    if (!p->workspace)
      return fail(MFA_ERR_INVALID_ARGUMENT, "workspace is required: mfa_mla_index_topk_launch keeps the logits in it, " + std::to_string(need) +
                                                " bytes (mfa_mla_index_workspace_size)");
    if (p->workspaceBytes < need)
      return fail(MFA_ERR_INVALID_ARGUMENT, "workspace too small: workspaceBytes = " + std::to_string(p->workspaceBytes) + ", the launch needs " +
                                                std::to_string(need) + " (mfa_mla_index_workspace_size)");
    if ((uintptr_t)p->workspace % 16 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    lrs = (int64_t)padded_column(p->column);
    lbs = lrs * p->rows;
  } else if ((st = check_index_logit_stride(p)) != MFA_OK) {
    return st;
  }
  grid = (uint32_t)(tiles * lists64);
  lists = (uint32_t)lists64;
  MlaIndexArgs &a = args;
  std::memset(&a, 0, sizeof(a));
  fill_index_args(a, p, pageShift);
  a.lrs = lrs; a.lbs = lbs;
  a.steps = (uint32_t)steps; a.tiles = (uint32_t)tiles;
  if (stage & LOGITS) logits = &kLogits[p->precision == MFA_FP16];
  if (stage == TOPK) a.logits = (float *)p->workspace;
  return MFA_OK;
}

mfa_status index_launch(int stage, const void *qi, const float *w, const void *ki, float *logits, int32_t *indices,
                        const mfa_mla_index_params *params, void *stream) {
  IndexPlan plan;
  mfa_status st = plan.prepare(params, stage);
  if (st == MFA_OK) st = bind_index(plan.args, stage, qi, w, ki, logits, indices);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status index_time(int stage, const void *qi, const float *w, const void *ki, float *logits, int32_t *indices,
                      const mfa_mla_index_params *params, void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  IndexPlan plan;
  mfa_status st = plan.prepare(params, stage);
  if (st == MFA_OK) st = bind_index(plan.args, stage, qi, w, ki, logits, indices);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

mfa_status index_launch_form(int stage, const mfa_mla_index_params *params, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  IndexPlan plan;
  const mfa_status st = plan.prepare(params, stage);
  if (st != MFA_OK) return st;
  const MlaIndexArgs &a = plan.args;
  char first[256] = "", second[128] = "";
  if (stage & LOGITS)
    std::snprintf(first, sizeof(first), "%s (grid %u = %u tiles of %u keys x %u rows x %u sequences, %u heads, %s)", plan.logits->name, plan.grid,
                  a.tiles, kTileKeys * a.steps, a.R, a.batches, a.H, a.paged ? "paged" : "contiguous");
  if (stage & SELECT)
    std::snprintf(second, sizeof(second), "%s (grid %u = %u rows x %u sequences, topk %u)", kSelect.name, plan.lists, a.R, a.batches, a.topk);
  const std::string text = std::string(first) + (stage == TOPK ? " + " : "") + second;
  copy_text(out, capacity, text.c_str());
  return MFA_OK;
}

} // namespace

extern "C" {

void mfa_mla_index_params_init(mfa_mla_index_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = MFA_BF16;
  params->indexDimension = MFA_MLA_INDEX_DIMENSION;
  params->causal = 1;
}

size_t mfa_mla_index_params_size(void) { return sizeof(mfa_mla_index_params); }

mfa_status mfa_mla_index_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_AT(FIELD) (uint32_t)offsetof(mfa_mla_index_params, FIELD)
  static const uint32_t table[] = {MFA_AT(rows), MFA_AT(column), MFA_AT(indexHeads), MFA_AT(batches), MFA_AT(causal), MFA_AT(indexDimension),
                                   MFA_AT(precision), MFA_AT(reserved), MFA_AT(pageSize), MFA_AT(topk), MFA_AT(cacheLengths), MFA_AT(blockTable),
                                   MFA_AT(blockTableStride), MFA_AT(leadingDimension), MFA_AT(headStride), MFA_AT(batchStride), MFA_AT(pageStride),
                                   MFA_AT(weightRowStride), MFA_AT(weightBatchStride), MFA_AT(logitRowStride), MFA_AT(logitBatchStride),
                                   MFA_AT(indexRowStride), MFA_AT(indexBatchStride), MFA_AT(workspace), MFA_AT(workspaceBytes)};
#undef MFA_AT
  const uint32_t fields = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = fields;
  for (uint32_t i = 0; i < fields && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_mla_index_workspace_size(const mfa_mla_index_params *params, uint64_t *bytes) {
  if (bytes) *bytes = 0;
  if (!bytes || !params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_mla_index_params probe = *params;   // every check of the chain but the workspace's own
  static float aligned[4] __attribute__((aligned(16)));
  probe.workspace = aligned;
  probe.workspaceBytes = ~0ull;
  IndexPlan plan;
  const mfa_status st = plan.prepare(&probe, TOPK);
  if (st != MFA_OK) return st;
  *bytes = workspace_bytes(params);
  return MFA_OK;
}

mfa_status mfa_mla_index_logits_launch(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                       void *stream) {
  return index_launch(LOGITS, qi, w, ki, logits, nullptr, params, stream);
}
mfa_status mfa_mla_index_logits_launch_form(const mfa_mla_index_params *params, char *out, size_t capacity) {
  return index_launch_form(LOGITS, params, out, capacity);
}
mfa_status mfa_mla_index_logits_time(const void *qi, const float *w, const void *ki, float *logits, const mfa_mla_index_params *params,
                                     void *stream, int warmup, int iterations, float *milliseconds) {
  return index_time(LOGITS, qi, w, ki, logits, nullptr, params, stream, warmup, iterations, milliseconds);
}

mfa_status mfa_mla_index_select_launch(const float *logits, int32_t *indices, const mfa_mla_index_params *params, void *stream) {
  return index_launch(SELECT, nullptr, nullptr, nullptr, const_cast<float *>(logits), indices, params, stream);
}
mfa_status mfa_mla_index_select_launch_form(const mfa_mla_index_params *params, char *out, size_t capacity) {
  return index_launch_form(SELECT, params, out, capacity);
}
mfa_status mfa_mla_index_select_time(const float *logits, int32_t *indices, const mfa_mla_index_params *params, void *stream, int warmup,
                                     int iterations, float *milliseconds) {
  return index_time(SELECT, nullptr, nullptr, nullptr, const_cast<float *>(logits), indices, params, stream, warmup, iterations, milliseconds);
}

mfa_status mfa_mla_index_topk_launch(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                     void *stream) {
  return index_launch(TOPK, qi, w, ki, nullptr, indices, params, stream);
}
mfa_status mfa_mla_index_topk_launch_form(const mfa_mla_index_params *params, char *out, size_t capacity) {
  return index_launch_form(TOPK, params, out, capacity);
}
mfa_status mfa_mla_index_topk_time(const void *qi, const float *w, const void *ki, int32_t *indices, const mfa_mla_index_params *params,
                                   void *stream, int warmup, int iterations, float *milliseconds) {
  return index_time(TOPK, qi, w, ki, nullptr, indices, params, stream, warmup, iterations, milliseconds);
}

} // extern "C"
