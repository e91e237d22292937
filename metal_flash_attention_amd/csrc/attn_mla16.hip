// attn_mla16.hip -- multi-head latent attention decode over a compressed KV cache: the kernels' code objects (attn_mla16.h), their
// tables and the C ABI of include/mfa_mla.h.  An entry of its own beside the decode and prefill launches: it stays out of their family
// tables.  Its checks, the argument block's shared fields, the piece plan (with decode's constants) and the entries' bodies are
// mla_launch.h's, which the other MLA units take too; what this unit adds is the dense packing, its grid and the dense launch form.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
// The decode entries of include/mfa_mla_cache.h over an e4m3 latent cache (attn_mla8.h) live here too: they are this plan with another
// kernel in front of the same combine kernel.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/mfa_mla.h"
#include "../../include/mfa_mla_cache.h"
#include "attn_mla16.h"
#include "attn_mla8.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla16_d576_<type> (unsplit), _k (a piece of the keys),
// _combine.  Two workgroups per compute unit: 64 KiB of LDS and at most 256 registers each.
#define MFA_MLA_KERNELS(TN, T)                                                                                                         \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla16_d576_##TN(const mfa::MlaArgs a) { mfa::mla_decode_body<T, false>(a); } \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla16_d576_##TN##_k(const mfa::MlaArgs a) { mfa::mla_decode_body<T, true>(a); } \
  extern "C" __global__ __launch_bounds__(256) void attn_mla16_d576_##TN##_combine(const mfa::MlaArgs a) { mfa::mla_combine_body<T>(a); }
MFA_MLA_KERNELS(bf16, __bf16)
MFA_MLA_KERNELS(f16, _Float16)
// ... and over an e4m3 latent cache: attn_mla8_d576_<type> and _k, merged by the combine kernel above
#define MFA_MLA8_KERNELS(TN, T)                                                                                                        \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla8_d576_##TN(const mfa::MlaArgs a) { mfa::mla8_decode_body<T, false>(a); } \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla8_d576_##TN##_k(const mfa::MlaArgs a) { mfa::mla8_decode_body<T, true>(a); }
MFA_MLA8_KERNELS(bf16, __bf16)
MFA_MLA8_KERNELS(f16, _Float16)

namespace {

typedef MlaKernelSet<MlaArgs> MlaSet;
#define MFA_MLA_SET(TN, PREC)                                                                                                         \
  {PREC, {MFA_CACHE_KERNEL(attn_mla16_d576_##TN), MFA_CACHE_KERNEL(attn_mla16_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla16_d576_##TN##_combine)}
const MlaSet kSets[] = {MFA_MLA_SET(bf16, MFA_BF16), MFA_MLA_SET(f16, MFA_FP16)};
#define MFA_MLA8_SET(TN, PREC)                                                                                                        \
  {PREC, {MFA_CACHE_KERNEL(attn_mla8_d576_##TN), MFA_CACHE_KERNEL(attn_mla8_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla16_d576_##TN##_combine)}
const MlaSet kSets8[] = {MFA_MLA8_SET(bf16, MFA_BF16), MFA_MLA8_SET(f16, MFA_FP16)};   // an e4m3 latent cache; the precision is Q's

// The dense plan: the packing is by (sequence, group of 32 packed rows), blocks = batches x groups, and the piece plan is over the
// 64-key tiles of `column`.
struct MlaPlan : MlaCutPlan<MlaArgs, MLA_LDS> {
  // `quant`: the block of the fp8_ entries, which they have checked (null: the entries of mfa_mla.h over a 16-bit cache)
  mfa_status prepare(const mfa_mla_decode_params *p, const mfa_mla_quant *quant) {
    uint32_t pageShift = 0;
    mfa_status st = check_mla_decode_params(p, quant != nullptr, &pageShift);
    if (st != MFA_OK) return st;
    const uint64_t M = (uint64_t)p->heads * p->rows, groups = (M + MFA_MLA_PACKED_ROWS - 1) / MFA_MLA_PACKED_ROWS;
    set = quant ? find_mla_set(kSets8, p->precision) : find_mla_set(kSets, p->precision);
    blocks = (uint32_t)(groups * p->batches);
    rows = (uint64_t)p->batches * M;
    std::memset(&args, 0, sizeof(args));
    fill_mla_args(args, p, pageShift);
    args.M = (uint32_t)M; args.groups = (uint32_t)groups;
    st = plan_mla_pieces(args, p->pieces, blocks, planned_tiles(p->column, p->rows, 0, 0), MFA_DECODE_WORKGROUP_TARGET, 4, MFA_DECODE_MAX_PIECES,
                         rows, p->workspace, p->workspaceBytes,
                         quant ? "mfa_attention_mla_decode_fp8_workspace_size" : "mfa_attention_mla_decode_workspace_size", &planned, &pieces);
    if (st != MFA_OK) return st;
    args.pieces = pieces;
    if (quant) args.kvScale = quant->kvScale;
    return MFA_OK;
  }
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args, args.kvScale, q, kv, o, l); }
};
// the plan of the fp8_ launch and time entries: the block is looked at first
struct Mla8Plan : MlaPlan {
  mfa_status prepare(const mfa_mla_decode_params *p, const mfa_mla_quant *quant) {
    const mfa_status st = check_mla_decode_quant(quant);
    return st != MFA_OK ? st : MlaPlan::prepare(p, quant);
  }
};

// ---- the bodies of the workspace_size and launch_form entries of both headers; `quant` as MlaPlan::prepare takes it
mfa_status mla_decode_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  if (!bytes || !params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  return mla_workspace_size<MlaPlan>(params, bytes, pieces, [quant](MlaPlan &plan, const mfa_mla_decode_params *probe) { return plan.prepare(probe, quant); });
}

mfa_status mla_decode_launch_form(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  MlaPlan plan;
  const mfa_status st = plan.prepare(params, quant);
  if (st != MFA_OK) return st;
  const MlaArgs &a = plan.args;
  const char *layout = a.paged ? "paged" : "contiguous";
  char text[512];
  if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u groups x %u sequences x %u pieces, %u packed rows, %s) + %s (grid %llu)", plan.name(),
                  plan.blocks * plan.pieces, a.groups, a.batches, plan.pieces, a.M, layout, plan.set->combine.name,
                  (unsigned long long)combine_grid(plan.rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u = %u groups x %u sequences, %u packed rows, %s%s)", plan.name(), plan.blocks, a.groups, a.batches,
                  a.M, layout, mla_unsplit_note(plan.planned).c_str());
  copy_text(out, capacity, text);
  return MFA_OK;
}

} // namespace

extern "C" {

void mfa_mla_decode_params_init(mfa_mla_decode_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->outputPrecision = MFA_BF16;
  params->headDimension = MFA_MLA_HEAD_DIMENSION;
  params->valueDimension = MFA_MLA_VALUE_DIMENSION;
  params->causal = 1;
}

size_t mfa_mla_decode_params_size(void) { return sizeof(mfa_mla_decode_params); }

mfa_status mfa_mla_decode_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_AT(FIELD) (uint32_t)offsetof(mfa_mla_decode_params, FIELD)
  static const uint32_t table[] = {MFA_AT(rows), MFA_AT(column), MFA_AT(heads), MFA_AT(batches), MFA_AT(causal), MFA_AT(headDimension),
                                   MFA_AT(valueDimension), MFA_AT(precision), MFA_AT(outputPrecision), MFA_AT(reserved), MFA_AT(scale),
                                   MFA_AT(pageSize), MFA_AT(pieces), MFA_AT(cacheLengths), MFA_AT(blockTable), MFA_AT(blockTableStride),
                                   MFA_AT(leadingDimension), MFA_AT(headStride), MFA_AT(batchStride), MFA_AT(pageStride), MFA_AT(lHeadStride),
                                   MFA_AT(lBatchStride), MFA_AT(workspace), MFA_AT(workspaceBytes)};
#undef MFA_AT
  const uint32_t fields = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = fields;
  for (uint32_t i = 0; i < fields && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_attention_mla_decode_workspace_size(const mfa_mla_decode_params *params, uint64_t *bytes, uint32_t *pieces) {
  return mla_decode_workspace_size(params, nullptr, bytes, pieces);
}

mfa_status mfa_attention_mla_decode_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                           void *stream) {
  return mla_launch<MlaPlan>(q, kv, o, l, stream, params, nullptr);
}

mfa_status mfa_attention_mla_decode_launch_form(const mfa_mla_decode_params *params, char *out, size_t capacity) {
  return mla_decode_launch_form(params, nullptr, out, capacity);
}

mfa_status mfa_attention_mla_decode_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                         void *stream, int warmup, int iterations, float *milliseconds) {
  return mla_time<MlaPlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params, nullptr);
}

// ---- include/mfa_mla_cache.h: the same four over an e4m3 latent cache.  The block is looked at first.
void mfa_mla_quant_init(mfa_mla_quant *quant) {
  if (!quant) return;
  std::memset(quant, 0, sizeof(*quant));
  quant->cachePrecision = MFA_KV_E4M3;
}

mfa_status mfa_attention_mla_decode_fp8_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, uint64_t *bytes,
                                                       uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  const mfa_status st = check_mla_decode_quant(quant);
  return st != MFA_OK ? st : mla_decode_workspace_size(params, quant, bytes, pieces);
}

mfa_status mfa_attention_mla_decode_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                               const mfa_mla_quant *quant, void *stream) {
  return mla_launch<Mla8Plan>(q, kv, o, l, stream, params, quant);
}

mfa_status mfa_attention_mla_decode_fp8_launch_form(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, char *out,
                                                    size_t capacity) {
  if (out && capacity) out[0] = '\0';
  const mfa_status st = check_mla_decode_quant(quant);
  return st != MFA_OK ? st : mla_decode_launch_form(params, quant, out, capacity);
}

mfa_status mfa_attention_mla_decode_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                             const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  return mla_time<Mla8Plan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params, quant);
}

} // extern "C"
