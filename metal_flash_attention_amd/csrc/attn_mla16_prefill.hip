// attn_mla16_prefill.hip -- multi-head latent attention prefill over the compressed KV cache: the kernels' code objects
// (attn_mla16_prefill.h) and the C ABI of include/mfa_mla_prefill.h.  An entry of its own beside attn_mla16.hip: it is in no family
// table, takes no option and no workspace, and takes from cache_launch.h what every launch over a cache shares -- the paging, stride,
// buffer and precision checks in their one wording and the timing loop.  What it refuses for the reason attn_mla16.hip refuses it, it
// refuses in that file's words.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_prefill.h"
#include "attn_mla16_prefill.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

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
  mfa_status prepare(const mfa_mla_prefill_params *p);
  hipError_t run(hipStream_t stream) const {
    const hipError_t err = launch_kernel(set->kernel.launch, dim3(grid), dim3(256), (uint32_t)MLAP_LDS, stream, args);
    return err != hipSuccess ? err : hipGetLastError();
  }
};

// every check that needs no GPU, and the kernel's argument block (the buffer pointers are filled in by the entries)
mfa_status MlaPrefillPlan::prepare(const mfa_mla_prefill_params *p) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, "MLA prefill reads 16-bit caches (MFA_BF16 or MFA_FP16); an FP32 cache has no kernel");
  mfa_status st = check_precisions(p->precision, p->outputPrecision);
  if (st != MFA_OK) return st;
  if (p->headDimension != MFA_MLA_HEAD_DIMENSION || p->valueDimension != MFA_MLA_VALUE_DIMENSION)
    return fail(MFA_ERR_UNSUPPORTED, "MLA prefill is compiled for (headDimension, valueDimension) = (576, 512), not (" +
                                         std::to_string(p->headDimension) + ", " + std::to_string(p->valueDimension) + ")");
  if (!(p->scale > 0.0f) || std::isinf(p->scale))   // (a NaN fails the comparison)
    return fail(MFA_ERR_INVALID_ARGUMENT, "scale is required: the model's softmax scale in natural units, finite and > 0 (there is no default), not " +
                                              std::to_string(p->scale));
  if ((st = check_sizes(p)) != MFA_OK) return st;
  const uint64_t M = (uint64_t)p->heads * p->rows, blocks = (M + MFA_MLA_PREFILL_PACKED_ROWS - 1) / MFA_MLA_PREFILL_PACKED_ROWS;
  if (M > 0x7FFFFFFFull || blocks * p->batches > 0x7FFFFFFFull)
    return fail(MFA_ERR_INVALID_ARGUMENT, "rows x heads, and blocks x batches, must fit a grid of 2^31 - 1 workgroups");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  uint32_t pageShift = 0;
  if ((st = check_paging(p->pageSize, p->blockTable, p->blockTableStride, p->column, &pageShift)) != MFA_OK) return st;
  static const char *names[3] = {"Q", "KV", "O"};
  for (int i = 0; i < 3; ++i) {
    const int64_t outer = i == 1 && p->pageSize ? p->pageStride : p->batchStride[i];
    st = check_operand_strides(names[i], i == 2 ? p->valueDimension : p->headDimension, p->leadingDimension[i], i == 1 ? 0 : p->headStride[i],
                               outer, i == 2 ? 4 : 8, "(16-byte rows for Q and KV; whole 4-element stores for O)");
    if (st != MFA_OK) return st;
  }
  set = nullptr;
  for (const MlaPrefillSet &s : kSets)
    if (s.precision == p->precision) set = &s;
  grid = (uint32_t)(blocks * p->batches);
  MlaPrefillArgs &a = args;
  std::memset(&a, 0, sizeof(a));
  a.lengths = p->cacheLengths;
  a.qlengths = p->queryLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride;
  a.ldo = p->leadingDimension[2]; a.hso = p->headStride[2]; a.bso = p->batchStride[2];
  a.lhs = p->lHeadStride; a.lbs = p->lBatchStride;
  a.R = p->rows; a.H = p->heads; a.blocks = (uint32_t)blocks; a.batches = p->batches; a.column = p->column;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0; a.outF32 = p->outputPrecision == MFA_FP32;
  a.scale2 = p->scale * 1.44269504089f;   // fl(scale x log2 e)
  return MFA_OK;
}

mfa_status bind_mla_prefill(MlaPrefillPlan *plan, const void *q, const void *kv, void *o, float *l) {
  mfa_status st = check_buffers({q, kv, o}, "Q, KV and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st != MFA_OK) return st;
  plan->args.q = (const char *)q; plan->args.kv = (const char *)kv; plan->args.o = (char *)o; plan->args.l = l;
  return MFA_OK;
}

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
  MlaPrefillPlan plan;
  mfa_status st = plan.prepare(params);
  if (st == MFA_OK) st = bind_mla_prefill(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_launch_form(const mfa_mla_prefill_params *params, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  MlaPrefillPlan plan;
  const mfa_status st = plan.prepare(params);
  if (st != MFA_OK) return st;
  const MlaPrefillArgs &a = plan.args;
  char text[512];
  std::snprintf(text, sizeof(text), "%s (grid %u = %u blocks x %u sequences, %llu packed rows in blocks of %d, %s)", plan.name(), plan.grid,
                a.blocks, a.batches, (unsigned long long)a.R * a.H, MFA_MLA_PREFILL_PACKED_ROWS, a.paged ? "paged" : "contiguous");
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                          void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  MlaPrefillPlan plan;
  mfa_status st = plan.prepare(params);
  if (st == MFA_OK) st = bind_mla_prefill(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

mfa_status mfa_attention_mla_prefill_step_range(uint32_t length, uint32_t queryLength, uint32_t firstPacked, uint32_t heads,
                                                uint32_t causal, uint32_t *firstMasked, uint32_t *end) {
  if (!firstMasked || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (heads == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "heads must be non-zero");
  mla_prefill_step_range(length, queryLength, firstPacked, heads, causal, firstMasked, end);
  return MFA_OK;
}

} // extern "C"
