// attn_mla8_prefill.hip -- multi-head latent attention prefill over an e4m3 latent cache: the kernels' code objects
// (attn_mla8_prefill.h) and the C ABI of include/mfa_mla_prefill_fp8.h, unsplit and cut along the keys.  A translation unit of its own,
// so that the kernels of attn_mla16_prefill.hip and attn_mla16_prefill_split.hip stay the code objects they are.  The order of the
// refusals is the header's: the quant block; the byte rows' strides; then, for the unsplit entries, everything the 16-bit plan refuses
// in its words (mla_prefill_prepare_args, attn_mla16_prefill_launch.h) and, for the cut entries, everything the 16-bit cut launch
// refuses about the split block and the params in its words, by handing both to mfa_attention_mla_prefill_split_workspace_size (which
// looks at no workspace and no GPU) -- that entry's piece count and byte count ARE this launch's: the plan and the workspace formula are
// not copied.  What this unit adds is the quant block's checks, the argument block and the launches.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN bytes past a length.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_prefill_fp8.h"
#include "attn_mla16_prefill_launch.h"
#include "attn_mla8_prefill.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

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

typedef CacheKernel<Mla8PrefillArgs> Mla8PrefillKernel;
struct Mla8PrefillSet {
  int precision;
  Mla8PrefillKernel kernel[2];   // [pieces > 1]
  Mla8PrefillKernel combine;
};
#define MFA_MLA8_PREFILL_SET(TN, PREC)                                                                                                 \
  {PREC, {MFA_CACHE_KERNEL(attn_mla8p_d576_##TN), MFA_CACHE_KERNEL(attn_mla8pk_d576_##TN)}, MFA_CACHE_KERNEL(attn_mla8p_d576_##TN##_combine)}
const Mla8PrefillSet kSets[] = {MFA_MLA8_PREFILL_SET(bf16, MFA_BF16), MFA_MLA8_PREFILL_SET(f16, MFA_FP16)};

// the quant block, looked at before everything else: required, e4m3, nothing reserved
mfa_status check_quant(const mfa_mla_quant *quant) {
  if (!quant)
    return fail(MFA_ERR_INVALID_ARGUMENT, "null mfa_mla_quant: the fp8 prefill entries require the block (mfa_mla_quant_init; a 16-bit latent "
                                          "cache: the mfa_mla_prefill.h entries)");
  bool fp8 = false;
  const mfa_status st = check_cache_precision(quant->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3, not " + std::to_string(quant->cachePrecision) +
                                              " (a 16-bit latent cache: the mfa_mla_prefill.h entries)");
  if (quant->reserved != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_quant.reserved must be 0, not " + std::to_string(quant->reserved));
  return MFA_OK;
}

struct Mla8PrefillPlan {
  Mla8PrefillArgs args;
  const Mla8PrefillSet *set;
  uint32_t pieces;      // as the launch runs: 1 for the unsplit entries and without a workspace
  uint32_t planned;     // what split->pieces asks for: the host's plan, or as given (the unsplit entries: 1)
  uint32_t blocks;      // batches x blocks of 64 packed rows: the unsplit grid
  uint64_t rows;        // batches x heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  uint64_t bytes;       // the workspace `planned` pieces need: the 16-bit cut launch's figure
  const Mla8PrefillKernel &kernel() const { return set->kernel[pieces > 1]; }
  const char *name() const { return kernel().name; }
  // `cut`: the split entries, which require `split`; otherwise `split` is not looked at
  mfa_status prepare(const mfa_mla_prefill_params *p, const mfa_key_split *split, bool cut, const mfa_mla_quant *quant);
  hipError_t run(hipStream_t stream) const {
    return run_pieces(kernel(), blocks, pieces, (uint32_t)MLAP_LDS, set->combine, rows, stream, args);
  }
};

// every check that needs no GPU, and the kernels' argument block (the buffer pointers are filled in by bind_mla8_prefill)
mfa_status Mla8PrefillPlan::prepare(const mfa_mla_prefill_params *p, const mfa_key_split *split, bool cut, const mfa_mla_quant *quant) {
  mfa_status st = check_quant(quant);
  if (st != MFA_OK) return st;
  // rows of bytes: a stride the 16-bit plan would take (a multiple of 8 elements) is not enough for a lane's 16-byte loads
  if (p && (st = check_stride_multiples("KV", p->leadingDimension[1], 0, p->pageSize ? p->pageStride : p->batchStride[1], 16,
                                        "(16-byte rows of an e4m3 cache)")) != MFA_OK)
    return st;
  bytes = 0;
  planned = 1;
  // the split block and the params as the 16-bit cut launch refuses them, with its plan's piece count
  if (cut && (st = mfa_attention_mla_prefill_split_workspace_size(p, split, &bytes, &planned)) != MFA_OK) return st;
  std::memset(&args, 0, sizeof(args));
  if ((st = mla_prefill_prepare_args(p, &args.a)) != MFA_OK) return st;
  set = nullptr;
  for (const Mla8PrefillSet &s : kSets)
    if (s.precision == p->precision) set = &s;
  blocks = args.a.blocks * args.a.batches;
  rows = (uint64_t)p->batches * p->heads * p->rows;
  pieces = cut && split->workspace ? planned : 1;   // no workspace: one kernel, unsplit
  if (pieces > 1) {
    st = check_split_workspace(split->workspace, split->workspaceBytes, bytes, "mfa_attention_mla_prefill_fp8_split_workspace_size");
    if (st != MFA_OK) return st;
    if ((uint64_t)blocks * pieces > 0x7FFFFFFFull)
      return fail(MFA_ERR_INVALID_ARGUMENT, "blocks x batches x pieces must fit a grid of 2^31 - 1 workgroups");
    set_split_slabs(args.a, split->workspace, pieces, rows, MLA_DV);
  }
  args.kvScale = quant->kvScale;
  return MFA_OK;
}

mfa_status bind_mla8_prefill(Mla8PrefillPlan *plan, const void *q, const void *kv, void *o, float *l) {
  mfa_status st = check_buffers({q, kv, o}, "Q, KV and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st == MFA_OK) st = check_float_arrays({plan->args.kvScale}, "kvScale");
  if (st != MFA_OK) return st;
  MlaPrefillArgs &a = plan->args.a;
  a.q = (const char *)q; a.kv = (const char *)kv; a.o = (char *)o; a.l = l;
  return MFA_OK;
}

// ---- the bodies of the entries of both families
mfa_status mla8_prefill_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                               const mfa_key_split *split, bool cut, const mfa_mla_quant *quant, void *stream) {
  Mla8PrefillPlan plan;
  mfa_status st = plan.prepare(params, split, cut, quant);
  if (st == MFA_OK) st = bind_mla8_prefill(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status mla8_prefill_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split, bool cut, const mfa_mla_quant *quant,
                                    char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  Mla8PrefillPlan plan;
  const mfa_status st = plan.prepare(params, split, cut, quant);
  if (st != MFA_OK) return st;
  const MlaPrefillArgs &a = plan.args.a;
  const char *layout = a.paged ? "paged" : "contiguous";
  char text[512];
  if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u blocks x %u sequences x %u pieces, %llu packed rows in blocks of %d, e4m3 cache, %s) + %s (grid %llu)",
                  plan.name(), plan.blocks * plan.pieces, a.blocks, a.batches, plan.pieces, (unsigned long long)a.R * a.H,
                  MFA_MLA_PREFILL_PACKED_ROWS, layout, plan.set->combine.name, (unsigned long long)combine_grid(plan.rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u = %u blocks x %u sequences, %llu packed rows in blocks of %d, e4m3 cache, %s%s)", plan.name(),
                  plan.blocks, a.blocks, a.batches, (unsigned long long)a.R * a.H, MFA_MLA_PREFILL_PACKED_ROWS, layout,
                  plan.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces").c_str() : "");
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mla8_prefill_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params, const mfa_key_split *split,
                             bool cut, const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  Mla8PrefillPlan plan;
  mfa_status st = plan.prepare(params, split, cut, quant);
  if (st == MFA_OK) st = bind_mla8_prefill(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

} // namespace

extern "C" {

mfa_status mfa_attention_mla_prefill_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                const mfa_mla_quant *quant, void *stream) {
  return mla8_prefill_launch(q, kv, o, l, params, nullptr, false, quant, stream);
}

mfa_status mfa_attention_mla_prefill_fp8_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_quant *quant, char *out,
                                                     size_t capacity) {
  return mla8_prefill_launch_form(params, nullptr, false, quant, out, capacity);
}

mfa_status mfa_attention_mla_prefill_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                              const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  return mla8_prefill_time(q, kv, o, l, params, nullptr, false, quant, stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_mla_prefill_fp8_split_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                      const mfa_key_split *split, const mfa_mla_quant *quant, void *stream) {
  return mla8_prefill_launch(q, kv, o, l, params, split, true, quant, stream);
}

mfa_status mfa_attention_mla_prefill_fp8_split_launch_form(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                           const mfa_mla_quant *quant, char *out, size_t capacity) {
  return mla8_prefill_launch_form(params, split, true, quant, out, capacity);
}

mfa_status mfa_attention_mla_prefill_fp8_split_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                    const mfa_key_split *split, const mfa_mla_quant *quant, void *stream, int warmup,
                                                    int iterations, float *milliseconds) {
  return mla8_prefill_time(q, kv, o, l, params, split, true, quant, stream, warmup, iterations, milliseconds);
}

mfa_status mfa_attention_mla_prefill_fp8_split_workspace_size(const mfa_mla_prefill_params *params, const mfa_key_split *split,
                                                              const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_key_split probe;
  if (split) {   // (the workspace the block may already name is not looked at)
    probe = *split;
    probe.workspace = nullptr;
    probe.workspaceBytes = 0;
  }
  Mla8PrefillPlan plan;
  const mfa_status st = plan.prepare(params, split ? &probe : nullptr, true, quant);
  if (st != MFA_OK) return st;
  *bytes = plan.bytes;
  if (pieces) *pieces = plan.planned;
  return MFA_OK;
}

} // extern "C"
