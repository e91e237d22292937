// attn_mla16_prefill_split.hip -- multi-head latent attention prefill CUT ALONG THE KEYS: the piece and combine kernels' code objects
// (the SPLIT side of attn_mla16_prefill.h) and the C ABI of include/mfa_mla_prefill_split.h.  A translation unit of its own beside
// attn_mla16_prefill.hip, so that the unsplit kernels' code objects stay what they were; a launch that is not cut -- one piece, or no
// workspace -- IS mfa_attention_mla_prefill_launch, and a parameter block is checked by that unit's plan in that unit's words
// (attn_mla16_prefill_launch.h).  From cache_launch.h: the piece count's formula, the workspace formula and its check, the slabs, the
// two launches of a run and the timing loop.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_prefill_split.h"
#include "attn_mla16_prefill_launch.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla16pk_d576_<type> (a piece of a block's keys) and
// attn_mla16p_d576_<type>_combine.  The piece kernel has the unsplit kernel's bound: 96 KiB of LDS, one workgroup a compute unit.
#define MFA_MLA_PREFILL_SPLIT_KERNELS(TN, T)                                                                                          \
  extern "C" __global__ __launch_bounds__(256, 1) void attn_mla16pk_d576_##TN(const mfa::MlaPrefillArgs a) { mfa::mla_prefill_body<T, true>(a); } \
  extern "C" __global__ __launch_bounds__(256) void attn_mla16p_d576_##TN##_combine(const mfa::MlaPrefillArgs a) { mfa::mla_prefill_combine_body<T>(a); }
MFA_MLA_PREFILL_SPLIT_KERNELS(bf16, __bf16)
MFA_MLA_PREFILL_SPLIT_KERNELS(f16, _Float16)

namespace {

typedef CacheKernel<MlaPrefillArgs> MlaPrefillKernel;
struct MlaPrefillSplitSet {
  int precision;
  MlaPrefillKernel piece, combine;
};
const MlaPrefillSplitSet kSets[] = {{MFA_BF16, MFA_CACHE_KERNEL(attn_mla16pk_d576_bf16), MFA_CACHE_KERNEL(attn_mla16p_d576_bf16_combine)},
                                    {MFA_FP16, MFA_CACHE_KERNEL(attn_mla16pk_d576_f16), MFA_CACHE_KERNEL(attn_mla16p_d576_f16_combine)}};

struct MlaPrefillSplitPlan {
  MlaPrefillArgs args;
  const MlaPrefillSplitSet *set;
  uint32_t pieces;      // as the launch runs: 1 without a workspace
  uint32_t planned;     // what split->pieces asks for: the host's plan, or as given
  uint32_t blocks;      // batches x blocks of 64 packed rows: the unsplit grid
  uint64_t rows;        // batches x heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  const char *name() const { return set->piece.name; }
  mfa_status prepare(const mfa_mla_prefill_params *p, const mfa_key_split *split);
  hipError_t run(hipStream_t stream) const {   // (pieces > 1 only)
    return run_pieces(set->piece, blocks, pieces, (uint32_t)MLAP_LDS, set->combine, rows, stream, args);
  }
};

// every check that needs no GPU: the split block's own, then the unsplit plan's, then the workspace's
mfa_status MlaPrefillSplitPlan::prepare(const mfa_mla_prefill_params *p, const mfa_key_split *split) {
  if (!split)
    return fail(MFA_ERR_INVALID_ARGUMENT, "null mfa_key_split: the split entries require the block (mfa_key_split_init; the launch that is "
                                          "never cut: mfa_attention_mla_prefill_launch)");
  if (split->pieces > MFA_MLA_PREFILL_SPLIT_MAX_PIECES)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_key_split.pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64 (a lane of the combine kernel's "
                                          "wave per piece), not " + std::to_string(split->pieces));
  if (split->reserved != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_key_split.reserved must be 0");
  mfa_status st = mla_prefill_prepare_args(p, &args);
  if (st != MFA_OK) return st;
  set = nullptr;
  for (const MlaPrefillSplitSet &s : kSets)
    if (s.precision == p->precision) set = &s;
  blocks = args.blocks * args.batches;
  rows = (uint64_t)p->batches * p->heads * p->rows;
  const uint64_t steps = ((uint64_t)p->column + MFA_MLA_PREFILL_KEY_STEP - 1) / MFA_MLA_PREFILL_KEY_STEP;
  planned = split->pieces ? split->pieces
                          : choose_pieces(blocks, steps, MFA_MLA_PREFILL_SPLIT_TARGET, MFA_MLA_PREFILL_SPLIT_MIN_STEPS, MFA_MLA_PREFILL_SPLIT_MAX_PIECES);
  pieces = split->workspace ? planned : 1;   // no workspace: one kernel, unsplit
  if (pieces > 1) {
    st = check_split_workspace(split->workspace, split->workspaceBytes, split_workspace_bytes(pieces, rows, MLA_DV),
                               "mfa_attention_mla_prefill_split_workspace_size");
    if (st != MFA_OK) return st;
    if ((uint64_t)blocks * pieces > 0x7FFFFFFFull)
      return fail(MFA_ERR_INVALID_ARGUMENT, "blocks x batches x pieces must fit a grid of 2^31 - 1 workgroups");
    set_split_slabs(args, split->workspace, pieces, rows, MLA_DV);
  }
  return MFA_OK;
}

mfa_status bind_split(MlaPrefillSplitPlan *plan, const void *q, const void *kv, void *o, float *l) {
  mfa_status st = check_buffers({q, kv, o}, "Q, KV and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st != MFA_OK) return st;
  plan->args.q = (const char *)q; plan->args.kv = (const char *)kv; plan->args.o = (char *)o; plan->args.l = l;
  return MFA_OK;
}

} // namespace

extern "C" {

mfa_status mfa_attention_mla_prefill_split_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                  const mfa_key_split *split, void *stream) {
  MlaPrefillSplitPlan plan;
  mfa_status st = plan.prepare(params, split);
  if (st != MFA_OK) return st;
  if (plan.pieces == 1) return mfa_attention_mla_prefill_launch(q, kv, o, l, params, stream);   // the unsplit launch, bit for bit
  if ((st = bind_split(&plan, q, kv, o, l)) != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_split_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split, char *out,
                                                       size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  MlaPrefillSplitPlan plan;
  mfa_status st = plan.prepare(params, split);
  if (st != MFA_OK) return st;
  const MlaPrefillArgs &a = plan.args;
  char text[512];
  if (plan.pieces > 1) {
    std::snprintf(text, sizeof(text), "%s (grid %u = %u blocks x %u sequences x %u pieces, %llu packed rows in blocks of %d, %s) + %s (grid %llu)",
                  plan.name(), plan.blocks * plan.pieces, a.blocks, a.batches, plan.pieces, (unsigned long long)a.R * a.H,
                  MFA_MLA_PREFILL_PACKED_ROWS, a.paged ? "paged" : "contiguous", plan.set->combine.name,
                  (unsigned long long)combine_grid(plan.rows));
  } else {   // the unsplit launch's own form, with the note where the plan would have cut
    if ((st = mfa_attention_mla_prefill_launch_form(params, text, sizeof(text))) != MFA_OK) return st;
    std::string form(text);
    if (plan.planned > 1 && !form.empty() && form.back() == ')') {
      form.pop_back();
      form += ", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces)";
    }
    std::snprintf(text, sizeof(text), "%s", form.c_str());
  }
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_split_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                const mfa_key_split *split, void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  MlaPrefillSplitPlan plan;
  mfa_status st = plan.prepare(params, split);
  if (st != MFA_OK) return st;
  if (plan.pieces == 1) return mfa_attention_mla_prefill_time(q, kv, o, l, params, stream, warmup, iterations, milliseconds);
  if ((st = bind_split(&plan, q, kv, o, l)) != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

mfa_status mfa_attention_mla_prefill_split_workspace_size(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                          uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_key_split probe;
  if (split) {   // (the workspace the block may already name is not looked at)
    probe = *split;
    probe.workspace = nullptr;
    probe.workspaceBytes = 0;
  }
  MlaPrefillSplitPlan plan;
  const mfa_status st = plan.prepare(params, split ? &probe : nullptr);
  if (st != MFA_OK) return st;
  if (plan.planned > 1) *bytes = split_workspace_bytes(plan.planned, plan.rows, MLA_DV);
  if (pieces) *pieces = plan.planned;
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_split_piece_range(uint32_t end, uint32_t pieces, uint32_t piece, uint32_t *beginStep,
                                                       uint32_t *endStep) {
  if (!beginStep || !endStep) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, and pieces non-zero");
  mla_prefill_split_piece_range(end, pieces, piece, beginStep, endStep);
  return MFA_OK;
}

} // extern "C"
