// attn_mla8_sparse.hip -- sparse MLA decode over an e4m3 latent cache: the kernels' code objects (attn_mla8_sparse.h) and the C ABI of
// include/mfa_mla_sparse_fp8.h.  A translation unit of its own, so that the kernels of attn_mla16.hip and attn_mla16_sparse.hip stay the
// code objects they are.  The order of the refusals is the header's: the sparse block in mfa_mla_sparse.h's words; then the quant block
// and everything the dense e4m3 plan refuses, in its words, by handing the params to mfa_attention_mla_decode_fp8_workspace_size (which
// looks at the quant block first and runs every check of its plan that needs neither a workspace nor a GPU); then the grid and the
// workspace.  What this unit adds is the packing by (sequence, row, group of heads), the plan over the slots and the argument block.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN bytes wherever no list points.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_sparse_fp8.h"
#include "attn_mla8_sparse.h"
#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"

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

typedef CacheKernel<MlaSparseArgs> SparseKernel;
struct SparseSet {
  int precision;
  SparseKernel kernel[2];   // [pieces > 1]
  SparseKernel combine;
};
#define MFA_MLA8_SPARSE_SET(TN, PREC)                                                                                                  \
  {PREC, {MFA_CACHE_KERNEL(attn_mla8x_d576_##TN), MFA_CACHE_KERNEL(attn_mla8x_d576_##TN##_k)}, MFA_CACHE_KERNEL(attn_mla8x_d576_##TN##_combine)}
const SparseSet kSets[] = {MFA_MLA8_SPARSE_SET(bf16, MFA_BF16), MFA_MLA8_SPARSE_SET(f16, MFA_FP16)};

// the sparse block, looked at before everything else: mfa_mla_sparse.h's requirements in its words
mfa_status check_sparse(const mfa_mla_sparse *s) {
  if (!s)
    return fail(MFA_ERR_INVALID_ARGUMENT, "null mfa_mla_sparse: the sparse entries require the block (mfa_mla_sparse_init; a launch over "
                                          "every key below the length: the mfa_mla.h entries)");
  if (!s->indices) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.indices is required (device array [batches][rows][topk] of int32 key positions)");
  if (s->topk == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.topk must be at least 1 (the slots of a row's list)");
  if (s->reserved != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.reserved must be 0, not " + std::to_string(s->reserved));
  if (s->indexRowStride < (int64_t)s->topk)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.indexRowStride must be at least topk = " + std::to_string(s->topk) + " entries, not " +
                                              std::to_string(s->indexRowStride));
  if ((uintptr_t)s->indices % 4 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_mla_sparse.indices must be 4-byte aligned");
  return MFA_OK;
}

struct Sparse8Plan {
  MlaSparseArgs args;
  const SparseSet *set;
  uint32_t pieces;      // as the launch runs: 1 without a workspace
  uint32_t planned;     // what params->pieces asks for: the host's plan, or as given
  uint32_t blocks;      // batches x rows x groups
  uint64_t rows;        // batches x heads x rows: the rows of a workspace slab, a wave of the combine kernel each
  const SparseKernel &kernel() const { return set->kernel[pieces > 1]; }
  const char *name() const { return kernel().name; }
  mfa_status prepare(const mfa_mla_decode_params *p, const mfa_mla_sparse *s, const mfa_mla_quant *quant);
  hipError_t run(hipStream_t stream) const {
    return run_pieces(kernel(), blocks, pieces, (uint32_t)MLA_LDS, set->combine, rows, stream, args);
  }
};

mfa_status Sparse8Plan::prepare(const mfa_mla_decode_params *p, const mfa_mla_sparse *s, const mfa_mla_quant *quant) {
  mfa_status st = check_sparse(s);
  if (st != MFA_OK) return st;
  // the quant block, then everything the dense e4m3 launch refuses for these params, both in its words (its workspace is its own
  // affair: the entry does not look at one)
  uint64_t denseBytes = 0;
  if ((st = mfa_attention_mla_decode_fp8_workspace_size(p, quant, &denseBytes, nullptr)) != MFA_OK) return st;
  const uint64_t groups = ((uint64_t)p->heads + MFA_MLA_PACKED_ROWS - 1) / MFA_MLA_PACKED_ROWS;
  const uint64_t wide = groups * p->rows * p->batches;
  if (wide * MFA_DECODE_MAX_PIECES > 0x7FFFFFFFull)
    return fail(MFA_ERR_INVALID_ARGUMENT, "groups x rows x batches x pieces must fit a grid of 2^31 - 1 workgroups");
  uint32_t pageShift = 0;
  if ((st = check_paging(p->pageSize, p->blockTable, p->blockTableStride, p->column, &pageShift)) != MFA_OK) return st;
  set = nullptr;
  for (const SparseSet &k : kSets)
    if (k.precision == p->precision) set = &k;
  blocks = (uint32_t)wide;
  rows = (uint64_t)p->batches * p->heads * p->rows;
  const uint64_t tiles = ((uint64_t)s->topk + MFA_DECODE_KEY_TILE - 1) / MFA_DECODE_KEY_TILE;
  planned = p->pieces ? p->pieces : choose_pieces(blocks, tiles, MFA_DECODE_WORKGROUP_TARGET, 4, MFA_DECODE_MAX_PIECES);
  pieces = planned;
  if (!p->workspace) pieces = 1;   // no workspace: one kernel, unsplit
  if (pieces > 1) {
    st = check_split_workspace(p->workspace, p->workspaceBytes, split_workspace_bytes(pieces, rows, MLA_DV),
                               "mfa_attention_mla_sparse_decode_fp8_workspace_size");
    if (st != MFA_OK) return st;
  }
  std::memset(&args, 0, sizeof(args));
  MlaArgs &a = args.a;
  a.lengths = p->cacheLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride;   // bytes
  a.ldo = p->leadingDimension[2]; a.hso = p->headStride[2]; a.bso = p->batchStride[2];
  a.lhs = p->lHeadStride; a.lbs = p->lBatchStride;
  a.R = p->rows; a.H = p->heads; a.M = p->heads * p->rows; a.groups = (uint32_t)groups; a.batches = p->batches; a.column = p->column;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0; a.outF32 = p->outputPrecision == MFA_FP32;
  a.scale2 = p->scale * 1.44269504089f;   // fl(scale x log2 e), as the dense launch forms it
  a.pieces = pieces;
  if (pieces > 1) set_split_slabs(a, p->workspace, pieces, rows, MLA_DV);
  a.kvScale = quant->kvScale;
  args.indices = s->indices;
  args.irs = s->indexRowStride;
  args.ibs = s->indexBatchStride;
  args.topk = s->topk;
  return MFA_OK;
}

mfa_status bind_sparse(Sparse8Plan *plan, const void *q, const void *kv, void *o, float *l) {
  mfa_status st = check_buffers({q, kv, o}, "Q, KV and O");
  if (st == MFA_OK) st = check_float_arrays({l}, "L");
  if (st == MFA_OK) st = check_float_arrays({plan->args.a.kvScale}, "kvScale");
  if (st != MFA_OK) return st;
  MlaArgs &a = plan->args.a;
  a.q = (const char *)q; a.kv = (const char *)kv; a.o = (char *)o; a.l = l;
  return MFA_OK;
}

} // namespace

extern "C" {

mfa_status mfa_attention_mla_sparse_decode_fp8_workspace_size(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse,
                                                              const mfa_mla_quant *quant, uint64_t *bytes, uint32_t *pieces) {
  if (bytes) *bytes = 0;
  if (pieces) *pieces = 0;
  mfa_status st = check_sparse(sparse);
  if (st != MFA_OK) return st;
  mfa_mla_decode_params probe;
  if (params) {
    probe = *params;
    probe.workspace = nullptr;
    probe.workspaceBytes = 0;
  }
  Sparse8Plan plan;
  if ((st = plan.prepare(params ? &probe : nullptr, sparse, quant)) != MFA_OK) return st;
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (plan.planned > 1) *bytes = split_workspace_bytes(plan.planned, plan.rows, MLA_DV);
  if (pieces) *pieces = plan.planned;
  return MFA_OK;
}

mfa_status mfa_attention_mla_sparse_decode_fp8_launch(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                      const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream) {
  Sparse8Plan plan;
  mfa_status st = plan.prepare(params, sparse, quant);
  if (st == MFA_OK) st = bind_sparse(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = plan.run((hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.name());
  return MFA_OK;
}

mfa_status mfa_attention_mla_sparse_decode_fp8_launch_form(const mfa_mla_decode_params *params, const mfa_mla_sparse *sparse,
                                                           const mfa_mla_quant *quant, char *out, size_t capacity) {
  if (out && capacity) out[0] = '\0';
  Sparse8Plan plan;
  mfa_status st = plan.prepare(params, sparse, quant);
  if (st != MFA_OK) return st;
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  const MlaArgs &a = plan.args.a;
  const char *layout = a.paged ? "paged" : "contiguous";
  char text[512];
  if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u groups x %u rows x %u sequences x %u pieces, topk %u, %s) + %s (grid %llu)", plan.name(),
                  plan.blocks * plan.pieces, a.groups, a.R, a.batches, plan.pieces, plan.args.topk, layout, plan.set->combine.name,
                  (unsigned long long)combine_grid(plan.rows));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u = %u groups x %u rows x %u sequences, topk %u, %s%s)", plan.name(), plan.blocks, a.groups, a.R,
                  a.batches, plan.args.topk, layout,
                  plan.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces").c_str() : "");
  copy_text(out, capacity, text);
  return MFA_OK;
}

mfa_status mfa_attention_mla_sparse_decode_fp8_time(const void *q, const void *kv, void *o, float *l, const mfa_mla_decode_params *params,
                                                    const mfa_mla_sparse *sparse, const mfa_mla_quant *quant, void *stream, int warmup,
                                                    int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  Sparse8Plan plan;
  mfa_status st = plan.prepare(params, sparse, quant);
  if (st == MFA_OK) st = bind_sparse(&plan, q, kv, o, l);
  if (st != MFA_OK) return st;
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan.name(), [&](hipStream_t s) { return plan.run(s); });
}

} // extern "C"
