// attn_mla8_sparse.hip -- sparse MLA decode over an e4m3 latent cache: the kernels' code objects (attn_mla8_sparse.h), their table and
// the C ABI of include/mfa_mla_sparse_fp8.h.  A translation unit of its own, so that the kernels of attn_mla16.hip and
// attn_mla16_sparse.hip stay the code objects they are.  The plan is mla_launch.h's MlaSparsePlan over this unit's kernels, with the
// header's order of refusals: the sparse block in mfa_mla_sparse.h's words; then the quant block and everything the dense e4m3 plan
// refuses, in its words; then the grid and the workspace.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN bytes wherever no list points.)
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/mfa_mla_sparse_fp8.h"
#include "attn_mla8_sparse.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla8x_d576_<type> (unsplit), _k (a piece of the slots),
// _combine (mla_combine_body, instantiated here: a kernel of another translation unit cannot be launched from this one without
// relocatable device code).  Two workgroups per compute unit, as the dense kernels.
#define MFA_MLA8_SPARSE_KERNELS(TN, T)                                                                                                 \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla8x_d576_##TN(const mfa::MlaSparseArgs a) {                             \
    mfa::mla8_sparse_decode_body<T, false>(a);                                                                                         \
  }                                                                                                                                    \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla8x_d576_##TN##_k(const mfa::MlaSparseArgs a) {                         \
    mfa::mla8_sparse_decode_body<T, true>(a);                                                                                          \
  }                                                                                                                                    \
  extern "C" __global__ __launch_bounds__(256) void attn_mla8x_d576_##TN##_combine(const mfa::MlaSparseArgs a) { mfa::mla_combine_body<T>(a.a); }
MFA_MLA8_SPARSE_KERNELS(bf16, __bf16)
MFA_MLA8_SPARSE_KERNELS(f16, _Float16)

namespace {

#define MFA_MLA8_SPARSE_SET(TN, PREC)                                                                                                  \
  {PREC, {MFA_CACHE_KERNEL(attn_mla8x_d576_##TN), MFA_CACHE_KERNEL(attn_mla8x_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla8x_d576_##TN##_combine)}
const MlaSparsePlan::Set kSets[] = {MFA_MLA8_SPARSE_SET(bf16, MFA_BF16), MFA_MLA8_SPARSE_SET(f16, MFA_FP16)};

} // namespace

extern "C" {

// (a NULL `params` is the plan's to refuse, after the blocks; a NULL `bytes` is judged after the plan)
mfa_status mfa_attention_mla_sparse_decode_fp8_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse,
                                                              const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  return mla_workspace_size<MlaSparsePlan>(params, bytes, pieces, [sparse, quant](MlaSparsePlan &plan, const mfa_mla_decode_params *probe) {
    return plan.prepare(kSets, true, probe, sparse, quant);
  });
}

mfa_status mfa_attention_mla_sparse_decode_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                      const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream) {
  return mla_launch<MlaSparsePlan>(q, kv, o, l, stream, kSets, true, params, sparse, quant);
}

// (a NULL `out` is judged after the plan)
mfa_status mfa_attention_mla_sparse_decode_fp8_launch_form(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse,
                                                           const mfa_mla_quant *quant, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  MlaSparsePlan plan;
  const mfa_status st = plan.prepare(kSets, true, params, sparse, quant);
  if (st != MFA_OK) return st;
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mla_sparse_decode_form(plan, out, capacity);
  return MFA_OK;
}

mfa_status mfa_attention_mla_sparse_decode_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                    const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream, int warmup,
                                                    int iterations, float *milliseconds) {
  return mla_time<MlaSparsePlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, kSets, true, params, sparse, quant);
}

} // extern "C"
