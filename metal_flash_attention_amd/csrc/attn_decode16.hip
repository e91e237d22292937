// attn_decode16.hip -- decode attention over a KV cache: the kernels' code objects and the C ABI of include/mfa_decode.h.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_decode.h"
#include "attn_decode16.h"
#include "attn_decode_plan.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

// Kernel names are plain C symbols, stable for a profiler's kernel trace: attn_decode16_d<D>_<type>_{single,pieces,combine}
#define MFA_DECODE_KERNELS(TN, T, D)                                                                                                  \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_decode16_d##D##_##TN##_single(const DecodeArgs a) {                       \
    decode16_body<T, D, false>(a);                                                                                                    \
  }                                                                                                                                   \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_decode16_d##D##_##TN##_pieces(const DecodeArgs a) {                       \
    decode16_body<T, D, true>(a);                                                                                                     \
  }                                                                                                                                   \
  extern "C" __global__ __launch_bounds__(256) void attn_decode16_d##D##_##TN##_combine(const DecodeArgs a) {                         \
    decode16_combine_body<T, D>(a);                                                                                                   \
  }
MFA_DECODE_KERNELS(bf16, __bf16, 64)
MFA_DECODE_KERNELS(bf16, __bf16, 128)
MFA_DECODE_KERNELS(f16, _Float16, 64)
MFA_DECODE_KERNELS(f16, _Float16, 128)

namespace {

typedef void (*DecodeKernel)(const DecodeArgs);
struct DecodeSet {
  uint32_t D;
  int precision;
  uint32_t lds;
  DecodeKernel single, pieces, combine;
  const char *singleName, *piecesName, *combineName;
};
#define MFA_DECODE_SET(TN, PREC, D)                                                                                                   \
  {D, PREC, (uint32_t)decode16_lds_bytes<D>(), attn_decode16_d##D##_##TN##_single, attn_decode16_d##D##_##TN##_pieces,                \
   attn_decode16_d##D##_##TN##_combine, "attn_decode16_d" #D "_" #TN "_single", "attn_decode16_d" #D "_" #TN "_pieces",              \
   "attn_decode16_d" #D "_" #TN "_combine"}
const DecodeSet kSets[] = {MFA_DECODE_SET(bf16, MFA_BF16, 64), MFA_DECODE_SET(bf16, MFA_BF16, 128), MFA_DECODE_SET(f16, MFA_FP16, 64),
                           MFA_DECODE_SET(f16, MFA_FP16, 128)};

mfa_status hip_fail(hipError_t err, const char *what) {
  return fail(MFA_ERR_HIP, std::string(what) + ": " + hipGetErrorName(err) + " (" + hipGetErrorString(err) + ")");
}

// Pieces of the keys: chosen from the workgroups the launch has without a split (batches x K/V heads) and `column` only -- the lengths
// live on the device.  Aims at MFA_DECODE_WORKGROUP_TARGET workgroups (two per compute unit of a 256-CU chip, what choose_splits of
// mfa_kernel.hip aims at), rounded down; a piece keeps at least four 64-key tiles (two steps for each of the workgroup's four waves)
uint32_t choose_pieces(uint64_t blocks, uint32_t column) {
  const uint64_t tiles = ((uint64_t)column + MFA_DECODE_KEY_TILE - 1) / MFA_DECODE_KEY_TILE;
  if (blocks >= MFA_DECODE_WORKGROUP_TARGET) return 1;
  uint64_t s = MFA_DECODE_WORKGROUP_TARGET / blocks;
  if (s > tiles / 4) s = tiles / 4;
  if (s > MFA_DECODE_MAX_PIECES) s = MFA_DECODE_MAX_PIECES;
  return s < 2 ? 1 : (uint32_t)s;
}

uint64_t pieces_workspace_bytes(uint32_t pieces, const mfa_decode_params *p) {
  return (uint64_t)pieces * p->batches * p->heads * p->rows * (p->headDimension + 2) * sizeof(float);
}

struct DecodePlan {
  DecodeArgs args;
  const DecodeSet *set;
  uint32_t pieces;      // as the launch runs: 1 without a workspace
  uint32_t planned;     // what the host would cut the keys into
  uint32_t blocks;      // batches x K/V heads
};

bool multiple_of(int64_t x, int64_t n) { return x % n == 0; }

// every check that needs no GPU, and the kernel's argument block (the buffer pointers are filled in by the launch)
mfa_status prepare(const mfa_decode_params *p, DecodePlan *plan) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention reads 16-bit caches (MFA_BF16 or MFA_FP16); an FP32 cache has no kernel");
  if (p->precision != MFA_BF16 && p->precision != MFA_FP16) return fail(MFA_ERR_INVALID_ARGUMENT, "precision must be MFA_FP16 or MFA_BF16");
  if (p->outputPrecision != p->precision && p->outputPrecision != MFA_FP32)
    return fail(MFA_ERR_INVALID_ARGUMENT, "outputPrecision must be the inputs' 16-bit type or MFA_FP32");
  const DecodeSet *set = nullptr;
  for (const DecodeSet &s : kSets)
    if (s.D == p->headDimension && s.precision == p->precision) set = &s;
  if (!set)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention is compiled for head dimensions 64 and 128, not " + std::to_string(p->headDimension));
  if (p->rows == 0 || p->column == 0 || p->heads == 0 || p->batches == 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "rows, column, heads and batches must be non-zero");
  const uint32_t G = p->headsPerKeyValue > 1 ? p->headsPerKeyValue : 1;
  if (p->heads % G != 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "heads (" + std::to_string(p->heads) + ") must be a multiple of headsPerKeyValue (" + std::to_string(G) + ")");
  if ((uint64_t)G * p->rows > MFA_DECODE_MAX_PACKED_ROWS)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention packs headsPerKeyValue x rows = " + std::to_string((uint64_t)G * p->rows) +
                                         " rows into one tile of at most 32; a longer block of query rows is a prefill: use "
                                         "mfa_attention_kernel_launch with headsPerKeyValue, columnLengths and causal");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  uint32_t pageShift = 0;
  if (p->pageSize) {
    if (p->pageSize < 16 || p->pageSize > 1024 || (p->pageSize & (p->pageSize - 1)))
      return fail(MFA_ERR_INVALID_ARGUMENT, "pageSize must be a power of two from 16 to 1024 (or 0: contiguous), not " + std::to_string(p->pageSize));
    if (!p->blockTable) return fail(MFA_ERR_INVALID_ARGUMENT, "a paged launch (pageSize != 0) needs blockTable");
    const int64_t pagesPerSequence = ((int64_t)p->column + p->pageSize - 1) / p->pageSize;
    if (p->blockTableStride < pagesPerSequence)
      return fail(MFA_ERR_INVALID_ARGUMENT, "blockTableStride must hold the " + std::to_string(pagesPerSequence) + " pages of `column` keys");
    while ((1u << pageShift) < p->pageSize) ++pageShift;
  }
  static const char *names[4] = {"Q", "K", "V", "O"};
  for (int i = 0; i < 4; ++i) {
    const int64_t need = (i == 3) ? 4 : 8;   // 16-byte rows of Q, K, V; 8- or 16-byte stores of O
    const bool kv = i == 1 || i == 2;
    if (p->leadingDimension[i] < (int64_t)p->headDimension)
      return fail(MFA_ERR_INVALID_ARGUMENT, std::string("leadingDimension of ") + names[i] + " is smaller than the head dimension");
    bool ok = multiple_of(p->leadingDimension[i], need) && multiple_of(p->headStride[i], need);
    if (!(kv && p->pageSize)) ok = ok && multiple_of(p->batchStride[i], need);
    if (kv && p->pageSize) ok = ok && multiple_of(p->pageStride[i - 1], need);
    if (!ok)
      return fail(MFA_ERR_INVALID_ARGUMENT, std::string("strides of ") + names[i] + " must be multiples of " + std::to_string(need) +
                                                " elements (16-byte rows for Q, K, V; whole 4-element stores for O)");
  }
  plan->set = set;
  plan->blocks = p->batches * (p->heads / G);
  plan->planned = choose_pieces(plan->blocks, p->column);
  plan->pieces = plan->planned;
  if (!p->workspace) plan->pieces = 1;   // no workspace: one kernel, unsplit
  if (plan->pieces > 1) {
    const uint64_t need = pieces_workspace_bytes(plan->pieces, p);
    if (p->workspaceBytes < need)
      return fail(MFA_ERR_INVALID_ARGUMENT, "workspace too small: " + std::to_string(p->workspaceBytes) + " bytes, the launch needs " +
                                                std::to_string(need) + " (mfa_attention_decode_workspace_size)");
    if ((uintptr_t)p->workspace % 16 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
  }
  DecodeArgs &a = plan->args;
  std::memset(&a, 0, sizeof(a));
  a.lengths = p->cacheLengths;
  a.table = p->blockTable;
  a.tableStride = p->blockTableStride;
  a.ldq = p->leadingDimension[0]; a.hsq = p->headStride[0]; a.bsq = p->batchStride[0];
  a.ldk = p->leadingDimension[1]; a.hsk = p->headStride[1]; a.bsk = p->batchStride[1]; a.psk = p->pageStride[0];
  a.ldv = p->leadingDimension[2]; a.hsv = p->headStride[2]; a.bsv = p->batchStride[2]; a.psv = p->pageStride[1];
  a.ldo = p->leadingDimension[3]; a.hso = p->headStride[3]; a.bso = p->batchStride[3];
  a.lhs = p->lHeadStride; a.lbs = p->lBatchStride;
  a.R = p->rows; a.G = G; a.Hq = p->heads; a.Hkv = p->heads / G; a.batches = p->batches; a.column = p->column;
  a.paged = p->pageSize != 0; a.pageShift = pageShift;
  a.causal = p->causal != 0; a.outF32 = p->outputPrecision == MFA_FP32;
  a.pieces = plan->pieces;
  a.scale2 = 1.44269504089f / std::sqrt((float)p->headDimension);
  if (plan->pieces > 1) {
    a.wsO = (float *)p->workspace;
    a.wsML = a.wsO + (uint64_t)plan->pieces * p->batches * p->heads * p->rows * p->headDimension;
  }
  return MFA_OK;
}

mfa_status bind(DecodePlan *plan, const void *q, const void *k, const void *v, void *o, float *l) {
  if (!q || !k || !v || !o) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if ((uintptr_t)q % 16 || (uintptr_t)k % 16 || (uintptr_t)v % 16 || (uintptr_t)o % 16)
    return fail(MFA_ERR_INVALID_ARGUMENT, "Q, K, V and O must be 16-byte aligned");
  if ((uintptr_t)l % 4) return fail(MFA_ERR_INVALID_ARGUMENT, "L must be 4-byte aligned");
  plan->args.q = (const char *)q; plan->args.k = (const char *)k; plan->args.v = (const char *)v;
  plan->args.o = (char *)o; plan->args.l = l;
  return MFA_OK;
}

hipError_t run(const DecodePlan &plan, hipStream_t stream) {
  const DecodeSet &s = *plan.set;
  hipError_t err;
  if (plan.pieces > 1) {
    err = launch_kernel(s.pieces, dim3(plan.blocks * plan.pieces), dim3(256), s.lds, stream, plan.args);
    if (err != hipSuccess) return err;
    const uint64_t rows = (uint64_t)plan.args.batches * plan.args.Hq * plan.args.R;
    err = launch_kernel(s.combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, stream, plan.args);
  } else {
    err = launch_kernel(s.single, dim3(plan.blocks), dim3(256), s.lds, stream, plan.args);
  }
  if (err != hipSuccess) return err;
  return hipGetLastError();
}

} // namespace

namespace mfa {

mfa_status decode_host_plan(const mfa_decode_params *params, DecodeHostPlan *out) {
  DecodePlan plan;
  const mfa_status st = prepare(params, &plan);
  if (st != MFA_OK) return st;
  out->args = plan.args;
  out->pieces = plan.pieces; out->planned = plan.planned; out->blocks = plan.blocks;
  out->lds = plan.set->lds;
  out->combine = plan.set->combine;
  out->combineName = plan.set->combineName;
  return MFA_OK;
}

uint64_t decode_workspace_bytes(uint32_t pieces, const mfa_decode_params *params) { return pieces_workspace_bytes(pieces, params); }

} // namespace mfa

extern "C" {

void mfa_decode_params_init(mfa_decode_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->outputPrecision = MFA_BF16;
  params->headsPerKeyValue = 1;
  params->causal = 1;
}

mfa_status mfa_attention_decode_piece_range(uint32_t length, uint32_t pieces, uint32_t piece, uint32_t *begin, uint32_t *end) {
  if (!begin || !end) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (pieces == 0 || piece >= pieces) return fail(MFA_ERR_INVALID_ARGUMENT, "piece must be below pieces, pieces non-zero");
  decode_piece_range(length, pieces, piece, begin, end);
  return MFA_OK;
}

mfa_status mfa_attention_decode_workspace_size(const mfa_decode_params *params, uint64_t *bytes) {
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = 0;
  if (!params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_decode_params probe = *params;   // the size does not depend on the workspace the caller may already have bound
  probe.workspace = nullptr;
  probe.workspaceBytes = 0;
  DecodePlan plan;
  const mfa_status st = prepare(&probe, &plan);
  if (st != MFA_OK) return st;
  if (plan.planned > 1) *bytes = pieces_workspace_bytes(plan.planned, params);
  return MFA_OK;
}

mfa_status mfa_attention_decode_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                       void *stream) {
  DecodePlan plan;
  mfa_status st = prepare(params, &plan);
  if (st != MFA_OK) return st;
  st = bind(&plan, q, k, v, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = run(plan, (hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.pieces > 1 ? plan.set->piecesName : plan.set->singleName);
  return MFA_OK;
}

mfa_status mfa_attention_decode_launch_form(const mfa_decode_params *params, char *out, size_t capacity) {
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  out[0] = '\0';
  DecodePlan plan;
  const mfa_status st = prepare(params, &plan);
  if (st != MFA_OK) return st;
  const DecodeSet &s = *plan.set;
  char text[512];
  const uint32_t M = plan.args.G * plan.args.R;
  if (plan.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u sequences x K/V heads x %u pieces, %u packed rows, %s) + %s (grid %llu)", s.piecesName,
                  plan.blocks * plan.pieces, plan.blocks, plan.pieces, M, plan.args.paged ? "paged" : "contiguous", s.combineName,
                  (unsigned long long)(((uint64_t)plan.args.batches * plan.args.Hq * plan.args.R + 3) / 4));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u sequences x K/V heads, %u packed rows, %s%s)", s.singleName, plan.blocks, M,
                  plan.args.paged ? "paged" : "contiguous",
                  plan.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(plan.planned) + " pieces").c_str() : "");
  std::strncpy(out, text, capacity - 1);
  out[capacity - 1] = '\0';
  return MFA_OK;
}

mfa_status mfa_attention_decode_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                     void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  DecodePlan plan;
  mfa_status st = prepare(params, &plan);
  if (st != MFA_OK) return st;
  st = bind(&plan, q, k, v, o, l);
  if (st != MFA_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t start, stop;
  hipError_t err = hipEventCreate(&start);
  if (err != hipSuccess) return hip_fail(err, "hipEventCreate");
  err = hipEventCreate(&stop);
  if (err != hipSuccess) { (void)hipEventDestroy(start); return hip_fail(err, "hipEventCreate"); }
  for (int i = 0; i < warmup && err == hipSuccess; ++i) err = run(plan, s);
  if (err == hipSuccess) err = hipEventRecord(start, s);
  for (int i = 0; i < iterations && err == hipSuccess; ++i) err = run(plan, s);
  if (err == hipSuccess) err = hipEventRecord(stop, s);
  if (err == hipSuccess) err = hipEventSynchronize(stop);
  if (err == hipSuccess) err = hipGetLastError();
  if (err == hipSuccess) err = hipEventElapsedTime(milliseconds, start, stop);
  (void)hipEventDestroy(start);
  (void)hipEventDestroy(stop);
  if (err != hipSuccess) return hip_fail(err, plan.set->singleName);
  return MFA_OK;
}

} // extern "C"
