// attn_mla8_prefill_sparse.hip -- sparse MLA prefill over an e4m3 latent cache: the kernels' code objects
// (attn_mla8_prefill_sparse.h), their table and the C ABI of include/mfa_mla_prefill_sparse_fp8.h.  A translation unit of its own, so
// that the kernels of attn_mla16_prefill_sparse.hip, attn_mla8_sparse.hip and attn_mla8_prefill.hip stay the code objects they are.
// The order of the refusals is the header's: the sparse block; the quant block; launch_form's buffer; everything the e4m3 prefill
// refuses for these params, in its words -- the byte rows' strides, then the 16-bit plan's checks --; then the grid.  Each of them is
// mla_launch.h's; what this unit adds is that order, the kernels and the cache's scale in the argument block.  No workspace, no pieces.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN bytes wherever no list points.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/mfa_mla_prefill_sparse_fp8.h"
#include "attn_mla8_prefill_sparse.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla8px1_d576_<type>, one tile -- 32 heads a workgroup,
// 64 KiB of LDS, two workgroups a compute unit -- at every head count.
#define MFA_MLA8_PREFILL_SPARSE_KERNELS(TN, T)                                                                                         \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla8px1_d576_##TN(const mfa::Mla8PrefillSparseArgs a) {                   \
    mfa::mla8_prefill_sparse_body<T>(a);                                                                                               \
  }
MFA_MLA8_PREFILL_SPARSE_KERNELS(bf16, __bf16)
MFA_MLA8_PREFILL_SPARSE_KERNELS(f16, _Float16)

namespace {

typedef CacheKernel<Mla8PrefillSparseArgs> Sparse8PrefillKernel;
struct Sparse8PrefillSet {
  int precision;
  Sparse8PrefillKernel kernel;
};
const Sparse8PrefillSet kSets[] = {{MFA_BF16, MFA_CACHE_KERNEL(attn_mla8px1_d576_bf16)}, {MFA_FP16, MFA_CACHE_KERNEL(attn_mla8px1_d576_f16)}};

struct Sparse8PrefillPlan {
  Mla8PrefillSparseArgs args;
  const Sparse8PrefillSet *set;
  uint32_t grid;   // batches x rows x groups
  const char *name() const { return set->kernel.name; }
  // (`out`: launch_form's buffer, refused after the blocks and ahead of the params; the launches pass none)
  mfa_status prepare(const mfa_mla_prefill_params *p, const mfa_mla_sparse *s, const mfa_mla_quant *quant, const char *const *out = nullptr);
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args.s.a, args.kvScale, q, kv, o, l); }
  hipError_t run(hipStream_t stream) const {
    const hipError_t err = launch_kernel(set->kernel.launch, dim3(grid), dim3(256), (uint32_t)MLA8PX_LDS, stream, args);
    return err != hipSuccess ? err : hipGetLastError();
  }
};

mfa_status Sparse8PrefillPlan::prepare(const mfa_mla_prefill_params *p, const mfa_mla_sparse *s, const mfa_mla_quant *quant,
                                       const char *const *out) {
  mfa_status st = check_mla_sparse(s, kMlaDensePrefill);
  if (st != MFA_OK) return st;
  if ((st = check_mla_quant(quant, "fp8 prefill", "mfa_mla_prefill.h", true)) != MFA_OK) return st;
  if (out && !*out) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  // everything the e4m3 prefill refuses for these params, in its words.  Rows of bytes: a stride the 16-bit plan would take (a
  // multiple of 8 elements) is not enough for a lane's 16-byte loads
  if (p && (st = check_stride_multiples("KV", p->leadingDimension[1], 0, p->pageSize ? p->pageStride : p->batchStride[1], 16,
                                        "(16-byte rows of an e4m3 cache)")) != MFA_OK)
    return st;
  std::memset(&args, 0, sizeof(args));
  MlaPrefillArgs &a = args.s.a;
  if ((st = prepare_mla_prefill_args(p, a)) != MFA_OK) return st;
  const uint64_t groups = ((uint64_t)p->heads + MLA_ROWS - 1) / MLA_ROWS;
  const uint64_t wide = groups * p->rows * p->batches;
  if (wide > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "groups x rows x batches must fit a grid of 2^31 - 1 workgroups");
  set = find_mla_set(kSets, p->precision);
  grid = (uint32_t)wide;
  a.blocks = (uint32_t)groups;   // the groups of heads of one (sequence, row), not prefill's blocks of packed rows
  args.s.indices = s->indices;
  args.s.irs = s->indexRowStride;
  args.s.ibs = s->indexBatchStride;
  args.s.topk = s->topk;
  args.kvScale = quant->kvScale;
  return MFA_OK;
}

} // namespace

extern "C" {

mfa_status mfa_attention_mla_prefill_sparse_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                       const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream) {
  return mla_launch<Sparse8PrefillPlan>(q, kv, o, l, stream, params, sparse, quant);
}

mfa_status mfa_attention_mla_prefill_sparse_fp8_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_sparse *sparse,
                                                            const mfa_mla_quant *quant, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  Sparse8PrefillPlan plan;
  const char *buffer = capacity ? out : nullptr;
  const mfa_status st = plan.prepare(params, sparse, quant, &buffer);
  if (st != MFA_OK) return st;
  const MlaPrefillArgs &a = plan.args.s.a;
  char text[512];
  std::snprintf(text, sizeof(text), "%s (grid %u = %u groups of %u heads x %u rows x %u sequences, topk %u, %s)", plan.name(), plan.grid, a.blocks,
                (unsigned)MLA_ROWS, a.R, a.batches, plan.args.s.topk, a.paged ? "paged" : "contiguous");
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_sparse_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                     const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream, int warmup,
                                                     int iterations, float *milliseconds) {
  return mla_time<Sparse8PrefillPlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params, sparse, quant);
}

} // extern "C"
