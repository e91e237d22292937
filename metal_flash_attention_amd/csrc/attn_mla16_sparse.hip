// attn_mla16_sparse.hip -- sparse MLA decode, the launch of mfa_mla.h over per-row lists of key positions: the kernels' code objects
// (attn_mla16_sparse.h), their table and the C ABI of include/mfa_mla_sparse.h.  A translation unit of its own, so that the kernels of
// attn_mla16.hip stay the code objects they are.  The plan is mla_launch.h's MlaSparsePlan over this unit's kernels: the block's checks,
// the dense launch's checks of the params in its words, the packing by (sequence, row, group of heads) and the plan over the slots.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN wherever no list points.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../include/mfa_mla_sparse.h"
#include "attn_mla16_sparse.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla16x_d576_<type> (unsplit), _k (a piece of the slots),
// _combine (mla_combine_body, instantiated here: a kernel of another translation unit cannot be launched from this one without
// relocatable device code).  Two workgroups per compute unit, as the dense kernels.
#define MFA_MLA_SPARSE_KERNELS(TN, T)                                                                                                  \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla16x_d576_##TN(const mfa::MlaSparseArgs a) {                            \
    mfa::mla_sparse_decode_body<T, false>(a);                                                                                          \
  }                                                                                                                                    \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla16x_d576_##TN##_k(const mfa::MlaSparseArgs a) {                        \
    mfa::mla_sparse_decode_body<T, true>(a);                                                                                           \
  }                                                                                                                                    \
  extern "C" __global__ __launch_bounds__(256) void attn_mla16x_d576_##TN##_combine(const mfa::MlaSparseArgs a) { mfa::mla_combine_body<T>(a.a); }
MFA_MLA_SPARSE_KERNELS(bf16, __bf16)
MFA_MLA_SPARSE_KERNELS(f16, _Float16)

namespace {

#define MFA_MLA_SPARSE_SET(TN, PREC)                                                                                                   \
  {PREC, {MFA_CACHE_KERNEL(attn_mla16x_d576_##TN), MFA_CACHE_KERNEL(attn_mla16x_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla16x_d576_##TN##_combine)}
const MlaSparsePlan::Set kSets[] = {MFA_MLA_SPARSE_SET(bf16, MFA_BF16), MFA_MLA_SPARSE_SET(f16, MFA_FP16)};

} // namespace

extern "C" {

void mfa_mla_sparse_init(mfa_mla_sparse *sparse) {
  if (sparse) std::memset(sparse, 0, sizeof(*sparse));
}

size_t mfa_mla_sparse_size(void) { return sizeof(mfa_mla_sparse); }

mfa_status mfa_mla_sparse_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_AT(FIELD) (uint32_t)offsetof(mfa_mla_sparse, FIELD)
  static const uint32_t table[] = {MFA_AT(indices), MFA_AT(topk), MFA_AT(reserved), MFA_AT(indexRowStride), MFA_AT(indexBatchStride)};
#undef MFA_AT
  const uint32_t fields = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = fields;
  for (uint32_t i = 0; i < fields && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

// (the block is looked at before a NULL `bytes` or `params`)
mfa_status mfa_attention_mla_sparse_decode_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse, uint64_t *bytes,
                                                          uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  const mfa_status st = check_mla_sparse(sparse, kMlaDenseDecode);
  if (st != MFA_OK) return st;
  if (!bytes || !params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  return mla_workspace_size<MlaSparsePlan>(params, bytes, pieces, [sparse](MlaSparsePlan &plan, const mfa_mla_decode_params *probe) {
    return plan.prepare(kSets, false, probe, sparse, nullptr);
  });
}

mfa_status mfa_attention_mla_sparse_decode_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                  const mfa_mla_sparse *sparse, void *stream) {
  return mla_launch<MlaSparsePlan>(q, kv, o, l, stream, kSets, false, params, sparse, nullptr);
}

// (the block is looked at before a NULL `out`)
mfa_status mfa_attention_mla_sparse_decode_launch_form(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse, char *out,
                                                       size_t capacity) {
  if (out && capacity) out[0] = '\0';
  MlaSparsePlan plan;
  mfa_status st = check_mla_sparse(sparse, kMlaDenseDecode);
  if (st != MFA_OK) return st;
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if ((st = plan.prepare(kSets, false, params, sparse, nullptr)) != MFA_OK) return st;
  mla_sparse_decode_form(plan, out, capacity);
  return MFA_OK;
}

mfa_status mfa_attention_mla_sparse_decode_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                const mfa_mla_sparse *sparse, void *stream, int warmup, int iterations, float *milliseconds) {
  return mla_time<MlaSparsePlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, kSets, false, params, sparse, nullptr);
}

} // extern "C"
