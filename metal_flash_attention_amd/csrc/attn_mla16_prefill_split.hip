// attn_mla16_prefill_split.hip -- multi-head latent attention prefill CUT ALONG THE KEYS: the piece and combine kernels' code objects
// (the SPLIT side of attn_mla16_prefill.h), their table and the C ABI of include/mfa_mla_prefill_split.h.  A translation unit of its own
// beside attn_mla16_prefill.hip, so that the unsplit kernels' code objects stay what they were; a launch that is not cut -- one piece,
// or no workspace -- IS mfa_attention_mla_prefill_launch.  The split block's checks, the unsplit launch's checks of the params in its
// words and the piece plan are mla_launch.h's; what this unit adds is their order and the kernels.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_prefill_split.h"
#include "attn_mla16_prefill.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla16pk_d576_<type> (a piece of a block's keys) and
// attn_mla16p_d576_<type>_combine.  The piece kernel has the unsplit kernel's bound: 96 KiB of LDS, one workgroup a compute unit.
#define MFA_MLA_PREFILL_SPLIT_KERNELS(TN, T)                                                                                          \
  extern "C" __global__ __launch_bounds__(256, 1) void attn_mla16pk_d576_##TN(const mfa::MlaPrefillArgs a) { mfa::mla_prefill_body<T, true>(a); } \
  extern "C" __global__ __launch_bounds__(256) void attn_mla16p_d576_##TN##_combine(const mfa::MlaPrefillArgs a) { mfa::mla_prefill_combine_body<T>(a); }
MFA_MLA_PREFILL_SPLIT_KERNELS(bf16, __bf16)
MFA_MLA_PREFILL_SPLIT_KERNELS(f16, _Float16)

namespace {

// (both kernels of a set name the piece kernel: the unsplit kernel is another unit's, and this plan runs only when it cuts)
#define MFA_MLA_PREFILL_SPLIT_SET(TN, PREC)                                                                                            \
  {PREC, {MFA_CACHE_KERNEL(attn_mla16pk_d576_##TN), MFA_CACHE_KERNEL(attn_mla16pk_d576_##TN)}, MFA_CACHE_KERNEL(attn_mla16p_d576_##TN##_combine)}
const MlaKernelSet<MlaPrefillArgs> kSets[] = {MFA_MLA_PREFILL_SPLIT_SET(bf16, MFA_BF16), MFA_MLA_PREFILL_SPLIT_SET(f16, MFA_FP16)};

struct MlaPrefillSplitPlan : MlaCutPlan<MlaPrefillArgs, MLAP_LDS> {   // (run: pieces > 1 only)
  // every check that needs no GPU: the split block's own, then the unsplit plan's, then the workspace's
  mfa_status prepare(const mfa_mla_prefill_params *p, const mfa_key_split *split) {
    mfa_status st = check_mla_prefill_split(split);
    if (st != MFA_OK) return st;
    std::memset(&args, 0, sizeof(args));
    if ((st = prepare_mla_prefill_args(p, args)) != MFA_OK) return st;
    set = find_mla_set(kSets, p->precision);
    return plan_mla_prefill_pieces(this, args, p, split, "mfa_attention_mla_prefill_split_workspace_size");
  }
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args, nullptr, q, kv, o, l); }
};

} // namespace

extern "C" {

mfa_status mfa_attention_mla_prefill_split_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                  const mfa_key_split *split, void *stream) {
  MlaPrefillSplitPlan plan;
  const mfa_status st = plan.prepare(params, split);
  if (st != MFA_OK) return st;
  if (plan.pieces == 1) return mfa_attention_mla_prefill_launch(q, kv, o, l, params, stream);   // the unsplit launch, bit for bit
  return mla_run(plan, q, kv, o, l, stream);
}

mfa_status mfa_attention_mla_prefill_split_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split, char *out,
                                                       size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  MlaPrefillSplitPlan plan;
  mfa_status st = plan.prepare(params, split);
  if (st != MFA_OK) return st;
  if (plan.pieces > 1) {
    mla_prefill_form(plan.name(), plan.args, plan.blocks, plan.pieces, plan.planned, plan.rows, "", plan.set->combine.name, out, capacity);
    return MFA_OK;
  }
  // the unsplit launch's own form, with the note where the plan would have cut
  char text[512];
  if ((st = mfa_attention_mla_prefill_launch_form(params, text, sizeof(text))) != MFA_OK) return st;
  std::string form(text);
  if (plan.planned > 1 && !form.empty() && form.back() == ')') {
    form.pop_back();
    form += mla_unsplit_note(plan.planned) + ")";
  }
  std::snprintf(text, sizeof(text), "%s", form.c_str());
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_split_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                const mfa_key_split *split, void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  MlaPrefillSplitPlan plan;
  const mfa_status st = plan.prepare(params, split);
  if (st != MFA_OK) return st;
  if (plan.pieces == 1) return mfa_attention_mla_prefill_time(q, kv, o, l, params, stream, warmup, iterations, milliseconds);
  return mla_time_run(plan, q, kv, o, l, stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_mla_prefill_split_workspace_size(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                          uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  return mla_workspace_size<MlaPrefillSplitPlan>(split, bytes, pieces, [params](MlaPrefillSplitPlan &plan, const mfa_key_split *probe) {
    return plan.prepare(params, probe);
  });
}

mfa_status mfa_attention_mla_prefill_split_piece_range(uint32_t end, uint32_t pieces, uint32_t piece, uint32_t *beginStep,
                                                       uint32_t *endStep) {
  if (!beginStep || !endStep) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, and pieces non-zero");
  mla_prefill_split_piece_range(end, pieces, piece, beginStep, endStep);
  return MFA_OK;
}

} // extern "C"
