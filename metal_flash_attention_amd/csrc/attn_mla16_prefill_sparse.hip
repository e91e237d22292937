// attn_mla16_prefill_sparse.hip -- sparse MLA prefill, the launch of mfa_mla_prefill.h over per-row lists of key positions: the kernels'
// code objects (attn_mla16_prefill_sparse.h), their table and the C ABI of include/mfa_mla_prefill_sparse.h.  A translation unit of its
// own, so that the kernels of attn_mla16_prefill.hip and attn_mla16_sparse.hip stay the code objects they are.  The block's checks and
// the dense prefill's checks of the params, in its words, are mla_launch.h's; what this unit adds is the packing by (sequence, row,
// group of heads), its grid and the list in the argument block.  No workspace, no pieces.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN wherever no list points.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/mfa_mla_prefill_sparse.h"
#include "attn_mla16_prefill_sparse.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "mla_launch.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_mla16px1_d576_<type>, one tile -- 32 heads a workgroup,
// 64 KiB of LDS, two workgroups a compute unit as the sparse decode -- at every head count.
// -DMFA_MLAPX_TWO_TILES builds the measured alternative, which lost (profiles/mla_sparse_prefill_perf.txt): launches
// of more than 32 heads run attn_mla16px_d576_<type>, two tiles -- 64 heads a workgroup, 96 KiB of LDS, one workgroup a compute unit.
#ifdef MFA_MLAPX_TWO_TILES
constexpr bool kTwoTiles = true;
#define MFA_MLA_PREFILL_SPARSE_KERNEL2(TN, T)                                                                                          \
  extern "C" __global__ __launch_bounds__(256, 1) void attn_mla16px_d576_##TN(const mfa::MlaPrefillSparseArgs a) {                    \
    mfa::mla_prefill_sparse_body<T, 2>(a);                                                                                             \
  }
#else
constexpr bool kTwoTiles = false;
#define MFA_MLA_PREFILL_SPARSE_KERNEL2(TN, T)
#endif
#define MFA_MLA_PREFILL_SPARSE_KERNELS(TN, T)                                                                                          \
  MFA_MLA_PREFILL_SPARSE_KERNEL2(TN, T)                                                                                                \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_mla16px1_d576_##TN(const mfa::MlaPrefillSparseArgs a) {                   \
    mfa::mla_prefill_sparse_body<T, 1>(a);                                                                                             \
  }
MFA_MLA_PREFILL_SPARSE_KERNELS(bf16, __bf16)
MFA_MLA_PREFILL_SPARSE_KERNELS(f16, _Float16)

namespace {

typedef CacheKernel<MlaPrefillSparseArgs> SparsePrefillKernel;
struct SparsePrefillSet {
  int precision;
  SparsePrefillKernel kernel[2];   // [tiles - 1]; without MFA_MLAPX_TWO_TILES both name the one-tile kernel
};
#ifdef MFA_MLAPX_TWO_TILES
#define MFA_MLA_PREFILL_SPARSE_SET(TN, PREC) {PREC, {MFA_CACHE_KERNEL(attn_mla16px1_d576_##TN), MFA_CACHE_KERNEL(attn_mla16px_d576_##TN)}}
#else
#define MFA_MLA_PREFILL_SPARSE_SET(TN, PREC) {PREC, {MFA_CACHE_KERNEL(attn_mla16px1_d576_##TN), MFA_CACHE_KERNEL(attn_mla16px1_d576_##TN)}}
#endif
const SparsePrefillSet kSets[] = {MFA_MLA_PREFILL_SPARSE_SET(bf16, MFA_BF16), MFA_MLA_PREFILL_SPARSE_SET(f16, MFA_FP16)};

struct SparsePrefillPlan {
  MlaPrefillSparseArgs args;
  const SparsePrefillSet *set;
  uint32_t tiles;    // 32-head tiles of a workgroup: 1 (2: the measured alternative)
  uint32_t grid;     // batches x rows x groups
  const SparsePrefillKernel &kernel() const { return set->kernel[tiles - 1]; }
  const char *name() const { return kernel().name; }
  // (`out`: launch_form's buffer, refused after the block and ahead of the params; the launches pass none)
  mfa_status prepare(const mfa_mla_prefill_params *p, const mfa_mla_sparse *s, const char *const *out = nullptr);
  mfa_status bind(const void *q, const void *kv, void *o, float *l) { return bind_mla(args.a, nullptr, q, kv, o, l); }
  hipError_t run(hipStream_t stream) const {
    const uint32_t lds = tiles == 1 ? (uint32_t)mlapx_lds<1>() : (uint32_t)mlapx_lds<2>();
    const hipError_t err = launch_kernel(kernel().launch, dim3(grid), dim3(256), lds, stream, args);
    return err != hipSuccess ? err : hipGetLastError();
  }
};

mfa_status SparsePrefillPlan::prepare(const mfa_mla_prefill_params *p, const mfa_mla_sparse *s, const char *const *out) {
  mfa_status st = check_mla_sparse(s, kMlaDensePrefill);
  if (st != MFA_OK) return st;
  if (out && !*out) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  // everything the dense prefill refuses for these params, in its words
  std::memset(&args, 0, sizeof(args));
  if ((st = prepare_mla_prefill_args(p, args.a)) != MFA_OK) return st;
  tiles = kTwoTiles && p->heads > (uint32_t)MLA_ROWS ? (uint32_t)MLAP_TILES : 1u;
  const uint64_t per = (uint64_t)tiles * MLA_ROWS, groups = ((uint64_t)p->heads + per - 1) / per;
  const uint64_t wide = groups * p->rows * p->batches;
  if (wide > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "groups x rows x batches must fit a grid of 2^31 - 1 workgroups");
  set = find_mla_set(kSets, p->precision);
  grid = (uint32_t)wide;
  args.a.blocks = (uint32_t)groups;   // the groups of heads of one (sequence, row), not prefill's blocks of packed rows
  args.indices = s->indices;
  args.irs = s->indexRowStride;
  args.ibs = s->indexBatchStride;
  args.topk = s->topk;
  return MFA_OK;
}

} // namespace

extern "C" {

mfa_status mfa_attention_mla_prefill_sparse_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                   const mfa_mla_sparse *sparse, void *stream) {
  return mla_launch<SparsePrefillPlan>(q, kv, o, l, stream, params, sparse);
}

mfa_status mfa_attention_mla_prefill_sparse_launch_form(const mfa_mla_prefill_params *params, const mfa_mla_sparse *sparse, char *out,
                                                        size_t capacity) {
  if (out && capacity) out[0] = '\0';
  SparsePrefillPlan plan;
  const char *buffer = capacity ? out : nullptr;
  const mfa_status st = plan.prepare(params, sparse, &buffer);
  if (st != MFA_OK) return st;
  const MlaPrefillArgs &a = plan.args.a;
  char text[512];
  std::snprintf(text, sizeof(text), "%s (grid %u = %u groups of %u heads x %u rows x %u sequences, topk %u, %s)", plan.name(), plan.grid, a.blocks,
                plan.tiles * MLA_ROWS, a.R, a.batches, plan.args.topk, a.paged ? "paged" : "contiguous");
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mfa_attention_mla_prefill_sparse_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_prefill_params *params,
                                                 const mfa_mla_sparse *sparse, void *stream, int warmup, int iterations, float *milliseconds) {
  return mla_time<SparsePrefillPlan>(q, kv, o, l, stream, warmup, iterations, milliseconds, params, sparse);
}

} // extern "C"
