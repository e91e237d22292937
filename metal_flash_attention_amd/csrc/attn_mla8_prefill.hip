// attn_mla8_prefill.hip -- multi-head latent attention prefill over an e4m3 latent cache: the kernels' code objects
// (attn_mla8_prefill.h), their table and the C ABI of include/mfa_mla_prefill_fp8.h, unsplit and cut along the keys.  A translation unit
// of its own, so that the kernels of attn_mla16_prefill.hip and attn_mla16_prefill_split.hip stay the code objects they are.  The order
// of the refusals is the header's: the quant block; the byte rows' strides; for the cut entries the split block; then everything the
// 16-bit plan refuses in its words; then the cut's workspace and grid -- each of them mla_launch.h's, as the 16-bit units take them.  What
// this unit adds is that order, the byte rows' rule, the kernels and the cache's scale in the argument block.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN bytes past a length.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../include/mfa_mla_prefill_fp8.h"
#include "attn_mla8_prefill.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla8p_d576_<type> (unsplit), attn_mla8pk_d576_<type> (a
// piece of a block's keys) and attn_mla8p_d576_<type>_combine (mla_prefill_combine_body, instantiated here: a kernel of another
// translation unit cannot be launched from this one without relocatable device code).  One workgroup a compute unit: 96 KiB of LDS.
#define MFA_MLA8_PREFILL_KERNELS(TN, T)                                                                                                \
  extern "C" __global__ __launch_bounds__(256, 1) void attn_mla8p_d576_##TN(const mfa::Mla8PrefillArgs a) {                           \
    mfa::mla8_prefill_body<T, false>(a);                                                                                               \
  }                                                                                                                                    \
  extern "C" __global__ __launch_bounds__(256, 1) void attn_mla8pk_d576_##TN(const mfa::Mla8PrefillArgs a) {                          \
    mfa::mla8_prefill_body<T, true>(a);                                                                                                \
  }                                                                                                                                    \
  extern "C" __global__ __launch_bounds__(256) void attn_mla8p_d576_##TN##_combine(const mfa::Mla8PrefillArgs a) {                    \
    mfa::mla_prefill_combine_body<T>(a.a);                                                                                             \
  }
MFA_MLA8_PREFILL_KERNELS(bf16, __bf16)
MFA_MLA8_PREFILL_KERNELS(f16, _Float16)

namespace {

#define MFA_MLA8_PREFILL_SET(TN, PREC)                                                                                                 \
  {PREC, {MFA_CACHE_KERNEL(attn_mla8p_d576_##TN), MFA_CACHE_KERNEL(attn_mla8pk_d576_##TN)}, MFA_CACHE_KERNEL(attn_mla8p_d576_##TN##_combine)}
const MlaKernelSet<Mla8PrefillArgs> kSets[] = {MFA_MLA8_PREFILL_SET(bf16, MFA_BF16), MFA_MLA8_PREFILL_SET(f16, MFA_FP16)};

struct Mla8PrefillPlan : MlaCutPlan<Mla8PrefillArgs, MLAP_LDS> {
  // every check that needs no GPU, and the kernels' argument block.  `cut`: the split entries, which require `split`; otherwise `split`
  // is not looked at and the launch is in one piece
  mfa_status prepare(const mfa_mla_prefill_params *p, const mfa_key_split *split, bool cut, const mfa_mla_quant *quant) {
    mfa_status st = check_mla_quant(quant, "fp8 prefill", "mfa_mla_prefill.h", true);
    if (st != MFA_OK) return st;
    // rows of bytes: a stride the 16-bit plan would take (a multiple of 8 elements) is not enough for a lane's 16-byte loads
    if (p && (st = check_stride_multiples("KV", p->leadingDimension[1], 0, p->pageSize ? p->pageStride : p->batchStride[1], 16,
                                          "(16-byte rows of an e4m3 cache)")) != MFA_OK)
      return st;
    if (cut && (st = check_mla_prefill_split(split)) != MFA_OK) return st;
    std::memset(&args, 0, sizeof(args));
    if ((st = prepare_mla_prefill_args(p, args.a)) != MFA_OK) return st;
    set = find_mla_set(kSets, p->precision);
    blocks = args.a.blocks * args.a.batches;
    rows = (uint64_t)p->batches * p->heads * p->rows;
    pieces = planned = 1;
    if (cut && (st = plan_mla_prefill_pieces(this, args.a, p, split, "mfa_attention_mla_prefill_fp8_split_workspace_size")) != MFA_OK) return st;
    args.kvScale = quant->kvScale;
    return MFA_OK;
  }
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args.a, args.kvScale, q, kv, o, l); }
};

// the body of the launch_form entries of both families
mfa_status mla8_prefill_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split, bool cut, const mfa_mla_quant *quant,
                                    char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  Mla8PrefillPlan plan;
  const mfa_status st = plan.prepare(params, split, cut, quant);
  if (st != MFA_OK) return st;
  mla_prefill_form(plan.name(), plan.args.a, plan.blocks, plan.pieces, plan.planned, plan.rows, "e4m3 cache, ", plan.set->combine.name, out, capacity);
  return MFA_OK;
}

} // namespace

extern "C" {

mfa_status mfa_attention_mla_prefill_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                const mfa_mla_quant *quant, void *stream) {
  return mla_launch<Mla8PrefillPlan>(q, kv, o, l, stream, params, nullptr, false, quant);
}

mfa_status mfa_attention_mla_prefill_fp8_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_quant *quant, char *out,
                                                     size_t capacity) {
  return mla8_prefill_launch_form(params, nullptr, false, quant, out, capacity);
}

mfa_status mfa_attention_mla_prefill_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                              const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  return mla_time<Mla8PrefillPlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params, nullptr, false, quant);
}

mfa_status mfa_attention_mla_prefill_fp8_split_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                      const mfa_key_split *split, const mfa_mla_quant *quant, void *stream) {
  return mla_launch<Mla8PrefillPlan>(q, kv, o, l, stream, params, split, true, quant);
}

mfa_status mfa_attention_mla_prefill_fp8_split_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                           const mfa_mla_quant *quant, char *out, size_t capacity) {
  return mla8_prefill_launch_form(params, split, true, quant, out, capacity);
}

mfa_status mfa_attention_mla_prefill_fp8_split_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                    const mfa_key_split *split, const mfa_mla_quant *quant, void *stream, int warmup,
                                                    int iterations, float *milliseconds) {
  return mla_time<Mla8PrefillPlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params, split, true, quant);
}

mfa_status mfa_attention_mla_prefill_fp8_split_workspace_size(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                              const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  return mla_workspace_size<Mla8PrefillPlan>(split, bytes, pieces, [params, quant](Mla8PrefillPlan &plan, const mfa_key_split *probe) {
    return plan.prepare(params, probe, true, quant);
  });
}

} // extern "C"
