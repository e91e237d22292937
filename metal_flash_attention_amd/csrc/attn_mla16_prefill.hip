// attn_mla16_prefill.hip -- multi-head latent attention prefill over the compressed KV cache: the kernels' code objects
// (attn_mla16_prefill.h), their table and the C ABI of include/mfa_mla_prefill.h.  An entry of its own beside attn_mla16.hip: it is in no
// family table and takes no option and no workspace.  Its checks and its argument block are mla_launch.h's prepare_mla_prefill_args,
// which the cut, e4m3 and sparse prefill units take too; what this unit adds is the kernel and its grid of batches x blocks.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../include/mfa_mla_prefill.h"
#include "attn_mla16_prefill.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla16p_d576_<type>.  One workgroup per compute unit:
// 96 KiB of LDS, and the two tiles' accumulators may live in the upper half of the 512 registers a lane then has.
#define MFA_MLA_PREFILL_KERNEL(TN, T)                                                                                                  \
  extern "C" __global__ __launch_bounds__(256, 1) void attn_mla16p_d576_##TN(const mfa::MlaPrefillArgs a) { mfa::mla_prefill_body<T>(a); }
MFA_MLA_PREFILL_KERNEL(bf16, __bf16)
MFA_MLA_PREFILL_KERNEL(f16, _Float16)

namespace {

typedef CacheKernel<MlaPrefillArgs> MlaPrefillKernel;
struct MlaPrefillSet {
  int precision;
  MlaPrefillKernel kernel;
};
const MlaPrefillSet kSets[] = {{MFA_BF16, MFA_CACHE_KERNEL(attn_mla16p_d576_bf16)}, {MFA_FP16, MFA_CACHE_KERNEL(attn_mla16p_d576_f16)}};

struct MlaPrefillPlan {
  MlaPrefillArgs args;
  const MlaPrefillSet *set;
  uint32_t grid;   // batches x blocks
  const char *name() const { return set->kernel.name; }
  mfa_status prepare(const mfa_mla_prefill_params *p) {
    std::memset(&args, 0, sizeof(args));
    const mfa_status st = prepare_mla_prefill_args(p, args);
    if (st != MFA_OK) return st;
    set = find_mla_set(kSets, p->precision);
    grid = args.blocks * args.batches;
    return MFA_OK;
  }
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args, nullptr, q, kv, o, l); }
  hipError_t run(hipStream_t stream) const {
    const hipError_t err = launch_kernel(set->kernel.launch, dim3(grid), dim3(256), (uint32_t)MLAP_LDS, stream, args);
    return err != hipSuccess ? err : hipGetLastError();
  }
};

} // namespace

extern "C" {

void mfa_mla_prefill_params_init(mfa_mla_prefill_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->outputPrecision = MFA_BF16;
  params->headDimension = MFA_MLA_HEAD_DIMENSION;
  params->valueDimension = MFA_MLA_VALUE_DIMENSION;
  params->causal = 1;
}

size_t mfa_mla_prefill_params_size(void) { return sizeof(mfa_mla_prefill_params); }

mfa_status mfa_mla_prefill_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_AT(FIELD) (uint32_t)offsetof(mfa_mla_prefill_params, FIELD)
  static const uint32_t table[] = {MFA_AT(rows), MFA_AT(column), MFA_AT(heads), MFA_AT(batches), MFA_AT(causal), MFA_AT(headDimension),
                                   MFA_AT(valueDimension), MFA_AT(precision), MFA_AT(outputPrecision), MFA_AT(reserved), MFA_AT(scale),
                                   MFA_AT(pageSize), MFA_AT(cacheLengths), MFA_AT(queryLengths), MFA_AT(blockTable), MFA_AT(blockTableStride),
                                   MFA_AT(leadingDimension), MFA_AT(headStride), MFA_AT(batchStride), MFA_AT(pageStride), MFA_AT(lHeadStride),
                                   MFA_AT(lBatchStride)};
#undef MFA_AT
  const uint32_t fields = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = fields;
  for (uint32_t i = 0; i < fields && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                            void *stream) {
  return mla_launch<MlaPrefillPlan>(q, kv, o, l, stream, params);
}

mfa_status mfa_attention_mla_prefill_launch_form(const mfa_mla_prefill_params *params, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  MlaPrefillPlan plan;
  const mfa_status st = plan.prepare(params);
  if (st != MFA_OK) return st;
  mla_prefill_form(plan.name(), plan.args, plan.grid, 1, 1, 0, "", nullptr, out, capacity);
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                          void *stream, int warmup, int iterations, float *milliseconds) {
  return mla_time<MlaPrefillPlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params);
}

mfa_status mfa_attention_mla_prefill_step_range(uint32_t length, uint32_t queryLength, uint32_t firstPacked, uint32_t heads,
                                                uint32_t causal, uint32_t *firstMasked, uint32_t *end) {
  if (!firstMasked || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (heads == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "heads must be non-zero");
  mla_prefill_step_range(length, queryLength, firstPacked, heads, causal, firstMasked, end);
  return MFA_OK;
}

} // extern "C"
