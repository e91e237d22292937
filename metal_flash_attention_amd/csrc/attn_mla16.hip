// attn_mla16.hip -- multi-head latent attention decode over a compressed KV cache: the kernels' code objects (attn_mla16.h) and the
// C ABI of include/mfa_mla.h.  An entry of its own beside the decode and prefill launches: it stays out of their family tables and
// takes from cache_launch.h what every launch over a cache shares -- the paging, stride, buffer and precision checks in their one
// wording, the piece count's formula (choose_pieces with decode's constants), the workspace formula, its check and the timing loop.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
// The decode entries of include/mfa_mla_cache.h over an e4m3 latent cache (attn_mla8.h) live here too: they are this plan with another
// kernel in front of the same combine kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla.h"
#include "../../include/mfa_mla_cache.h"
#include "attn_mla16.h"
#include "attn_mla8.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

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

typedef CacheKernel<MlaArgs> MlaKernel;
struct MlaSet {
  int precision;
  MlaKernel kernel[2];   // [pieces > 1]
  MlaKernel combine;
};
#define MFA_MLA_SET(TN, PREC)                                                                                                         \
  {PREC, {MFA_CACHE_KERNEL(attn_mla16_d576_##TN), MFA_CACHE_KERNEL(attn_mla16_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla16_d576_##TN##_combine)}
const MlaSet kSets[] = {MFA_MLA_SET(bf16, MFA_BF16), MFA_MLA_SET(f16, MFA_FP16)};
#define MFA_MLA8_SET(TN, PREC)                                                                                                        \
  {PREC, {MFA_CACHE_KERNEL(attn_mla8_d576_##TN), MFA_CACHE_KERNEL(attn_mla8_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla16_d576_##TN##_combine)}
const MlaSet kSets8[] = {MFA_MLA8_SET(bf16, MFA_BF16), MFA_MLA8_SET(f16, MFA_FP16)};   // an e4m3 latent cache; the precision is Q's

struct MlaPlan {
  MlaArgs args;
  const MlaSet *set;
  uint32_t pieces;      // as the launch runs: 1 without a workspace
  uint32_t planned;     // what params->pieces asks for: the host's plan, or as given
  uint32_t blocks;      // batches x groups
  uint64_t rows;        // batches x heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  const MlaKernel &kernel() const { return set->kernel[pieces > 1]; }
  const char *name() const { return kernel().name; }
  // `quant`: the block of the fp8_ entries, checked by check_quant (null: the entries of mfa_mla.h over a 16-bit cache)
  mfa_status prepare(const mfa_mla_decode_params *p, const mfa_mla_quant *quant = nullptr);
  hipError_t run(hipStream_t stream) const {
    return run_pieces(kernel(), blocks, pieces, (uint32_t)MLA_LDS, set->combine, rows, stream, args);
  }
};

// every check that needs no GPU, and the kernel's argument block (the buffer pointers are filled in by the entries)
mfa_status MlaPlan::prepare(const mfa_mla_decode_params *p, const mfa_mla_quant *quant) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, quant ? "MLA decode over an e4m3 latent cache takes a 16-bit Q (precision MFA_BF16 or MFA_FP16); an FP32 Q has no kernel"
                                           : "MLA decode reads 16-bit caches (MFA_BF16 or MFA_FP16); an FP32 cache has no kernel");
  mfa_status st = check_precisions(p->precision, p->outputPrecision);
  if (st != MFA_OK) return st;
  if (p->headDimension != MFA_MLA_HEAD_DIMENSION || p->valueDimension != MFA_MLA_VALUE_DIMENSION)
    return fail(MFA_ERR_UNSUPPORTED, "MLA decode is compiled for (headDimension, valueDimension) = (576, 512), not (" +
                                         std::to_string(p->headDimension) + ", " + std::to_string(p->valueDimension) + ")");
  if (!(p->scale > 0.0f) || std::isinf(p->scale))   // (a NaN fails the comparison)
    return fail(MFA_ERR_INVALID_ARGUMENT, "scale is required: the model's softmax scale in natural units, finite and > 0 (there is no default), not " +
                                              std::to_string(p->scale));
  if ((st = check_sizes(p)) != MFA_OK) return st;
  if (p->rows > MFA_MLA_PACKED_ROWS)
    return fail(MFA_ERR_UNSUPPORTED, "MLA decode takes at most 32 rows per sequence, not " + std::to_string(p->rows) +
                                         ": a longer block of query rows is a prefill, which is not served over the latent cache");
  if (p->pieces > MFA_DECODE_MAX_PIECES)
    return fail(MFA_ERR_INVALID_ARGUMENT, "pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. " + std::to_string(MFA_DECODE_MAX_PIECES) +
                                              ", not " + std::to_string(p->pieces));
  const uint64_t M = (uint64_t)p->heads * p->rows, groups = (M + MFA_MLA_PACKED_ROWS - 1) / MFA_MLA_PACKED_ROWS;
  if (M > 0x7FFFFFFFull || groups * p->batches * MFA_DECODE_MAX_PIECES > 0x7FFFFFFFull)
    return fail(MFA_ERR_INVALID_ARGUMENT, "groups x batches x pieces must fit a grid of 2^31 - 1 workgroups");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  uint32_t pageShift = 0;
  if ((st = check_paging(p->pageSize, p->blockTable, p->blockTableStride, p->column, &pageShift)) != MFA_OK) return st;
  static const char *names[3] = {"Q", "KV", "O"};
  for (int i = 0; i < 3; ++i) {
    const int64_t outer = i == 1 && p->pageSize ? p->pageStride : p->batchStride[i];
    const bool bytes = i == 1 && quant;   // rows of an e4m3 cache: an element is a byte
    st = check_operand_strides(names[i], i == 2 ? p->valueDimension : p->headDimension, p->leadingDimension[i], i == 1 ? 0 : p->headStride[i],
                               outer, i == 2 ? 4 : bytes ? 16 : 8,
                               bytes ? "(16-byte rows of an e4m3 cache)" : "(16-byte rows for Q and KV; whole 4-element stores for O)");
    if (st != MFA_OK) return st;
  }
  set = nullptr;
  for (const MlaSet &s : quant ? kSets8 : kSets)
    if (s.precision == p->precision) set = &s;
  blocks = (uint32_t)(groups * p->batches);
  rows = (uint64_t)p->batches * M;
  const uint64_t tiles = planned_tiles(p->column, p->rows, 0, 0);
  planned = p->pieces ? p->pieces : choose_pieces(blocks, tiles, MFA_DECODE_WORKGROUP_TARGET, 4, MFA_DECODE_MAX_PIECES);
  pieces = planned;
  if (!p->workspace) pieces = 1;   // no workspace: one kernel, unsplit
  if (pieces > 1) {
    st = check_split_workspace(p->workspace, p->workspaceBytes, split_workspace_bytes(pieces, rows, MLA_DV),
                               quant ? "mfa_attention_mla_decode_fp8_workspace_size" : "mfa_attention_mla_decode_workspace_size");
    if (st != MFA_OK) return st;
  }
  MlaArgs &a = args;
  std::memset(&a, 0, sizeof(a));
  a.lengths = p->cacheLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride;
  a.ldo = p->leadingDimension[2]; a.hso = p->headStride[2]; a.bso = p->batchStride[2];
  a.lhs = p->lHeadStride; a.lbs = p->lBatchStride;
  a.R = p->rows; a.H = p->heads; a.M = (uint32_t)M; a.groups = (uint32_t)groups; a.batches = p->batches; a.column = p->column;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0; a.outF32 = p->outputPrecision == MFA_FP32;
  a.scale2 = p->scale * 1.44269504089f;   // fl(scale x log2 e)
  a.pieces = pieces;
  if (pieces > 1) set_split_slabs(a, p->workspace, pieces, rows, MLA_DV);
  if (quant) a.kvScale = quant->kvScale;
  return MFA_OK;
}

// the block of the fp8_ entries (include/mfa_mla_cache.h): required, and its cache is e4m3
mfa_status check_quant(const mfa_mla_quant *quant) {
  if (!quant)
    return fail(MFA_ERR_INVALID_ARGUMENT, "null mfa_mla_quant: the fp8 entries require the block (mfa_mla_quant_init; a 16-bit latent "
                                          "cache: the mfa_mla.h entries)");
  bool fp8 = false;
  const mfa_status st = check_cache_precision(quant->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3, not " + std::to_string(quant->cachePrecision) +
                                              " (a 16-bit latent cache: the mfa_mla.h entries)");
  return MFA_OK;
}

mfa_status bind_mla(MlaPlan *plan, const void *q, const void *kv, void *o, float *l) {
  mfa_status st = check_buffers({q, kv, o}, "Q, KV and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st == MFA_OK) st = check_float_arrays({plan->args.kvScale}, "kvScale");
  if (st != MFA_OK) return st;
  plan->args.q = (const char *)q; plan->args.kv = (const char *)kv; plan->args.o = (char *)o; plan->args.l = l;
  return MFA_OK;
}

// ---- the bodies of the entries of both headers; `quant` as prepare takes it
mfa_status mla_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  if (!bytes || !params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_mla_decode_params probe = *params;
  probe.workspace = nullptr;
  probe.workspaceBytes = 0;
  MlaPlan plan;
  const mfa_status st = plan.prepare(&probe, quant);
  if (st != MFA_OK) return st;
  if (plan.planned > 1) *bytes = split_workspace_bytes(plan.planned, plan.rows, MLA_DV);
  if (pieces) *pieces = plan.planned;
  return MFA_OK;
}

mfa_status mla_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params, const mfa_mla_quant *quant,
                      void *stream) {
  MlaPlan plan;
  mfa_status st = plan.prepare(params, quant);
  if (st == MFA_OK) st = bind_mla(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status mla_launch_form(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, char *out, size_t capacity) {
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
                  a.M, layout,
                  plan.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces").c_str() : "");
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mla_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params, const mfa_mla_quant *quant,
                    void *stream, int warmup, int iterations, float *milliseconds) {
  MlaPlan plan;
  mfa_status st = plan.prepare(params, quant);
  if (st == MFA_OK) st = bind_mla(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
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
  return mla_workspace_size(params, nullptr, bytes, pieces);
}

mfa_status mfa_attention_mla_decode_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                           void *stream) {
  return mla_launch(q, kv, o, l, params, nullptr, stream);
}

mfa_status mfa_attention_mla_decode_launch_form(const mfa_mla_decode_params *params, char *out, size_t capacity) {
  return mla_launch_form(params, nullptr, out, capacity);
}

mfa_status mfa_attention_mla_decode_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                         void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  return mla_time(q, kv, o, l, params, nullptr, stream, warmup, iterations, milliseconds);
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
  const mfa_status st = check_quant(quant);
  return st != MFA_OK ? st : mla_workspace_size(params, quant, bytes, pieces);
}

mfa_status mfa_attention_mla_decode_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                               const mfa_mla_quant *quant, void *stream) {
  const mfa_status st = check_quant(quant);
  return st != MFA_OK ? st : mla_launch(q, kv, o, l, params, quant, stream);
}

mfa_status mfa_attention_mla_decode_fp8_launch_form(const mfa_mla_decode_params *params, const mfa_mla_quant *quant, char *out,
                                                    size_t capacity) {
  if (out && capacity) out[0] = '\0';
  const mfa_status st = check_quant(quant);
  return st != MFA_OK ? st : mla_launch_form(params, quant, out, capacity);
}

mfa_status mfa_attention_mla_decode_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                             const mfa_mla_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  const mfa_status st = check_quant(quant);
  return st != MFA_OK ? st : mla_time(q, kv, o, l, params, quant, stream, warmup, iterations, milliseconds);
}

} // extern "C"
