// attn_decode8.hip -- decode attention over an FP8 (e4m3) KV cache: the kernels' code objects and the decode entries of
// include/mfa_kvcache.h.  The plan -- checks, piece count, workspace, combine kernel -- is the 16-bit launch's (attn_decode_plan.h).
// (Not named attn_fwd16*: compiled without -ffinite-math-only, as attn_decode16.hip is.)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mfa_kvcache.h"
#include "attn_decode8.h"
#include "attn_decode_plan.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

// attn_decode8_d<D>_<type of Q>_{single,pieces}; the pieces are merged by attn_decode16_d<D>_<type>_combine
#define MFA_DECODE8_KERNELS(TN, T, D)                                                                                                 \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_decode8_d##D##_##TN##_single(const DecodeArgs a, const float *ks,         \
                                                                                         const float *vs) {                          \
    decode8_body<T, D, false>(a, ks, vs);                                                                                             \
  }                                                                                                                                   \
  extern "C" __global__ __launch_bounds__(256, 2) void attn_decode8_d##D##_##TN##_pieces(const DecodeArgs a, const float *ks,         \
                                                                                         const float *vs) {                          \
    decode8_body<T, D, true>(a, ks, vs);                                                                                              \
  }
MFA_DECODE8_KERNELS(bf16, __bf16, 64)
MFA_DECODE8_KERNELS(bf16, __bf16, 128)
MFA_DECODE8_KERNELS(f16, _Float16, 64)
MFA_DECODE8_KERNELS(f16, _Float16, 128)

namespace {

typedef void (*Decode8Kernel)(const DecodeArgs, const float *, const float *);
struct Decode8Set {
  uint32_t D;
  int precision;
  Decode8Kernel single, pieces;
  const char *singleName, *piecesName;
};
#define MFA_DECODE8_SET(TN, PREC, D)                                                                                                  \
  {D, PREC, attn_decode8_d##D##_##TN##_single, attn_decode8_d##D##_##TN##_pieces, "attn_decode8_d" #D "_" #TN "_single",              \
   "attn_decode8_d" #D "_" #TN "_pieces"}
const Decode8Set kSets[] = {MFA_DECODE8_SET(bf16, MFA_BF16, 64), MFA_DECODE8_SET(bf16, MFA_BF16, 128), MFA_DECODE8_SET(f16, MFA_FP16, 64),
                            MFA_DECODE8_SET(f16, MFA_FP16, 128)};

struct Plan8 {
  DecodeHostPlan host;
  const Decode8Set *set;
  const float *keyScale, *valueScale;
};

mfa_status hip_fail(hipError_t err, const char *what) {
  return fail(MFA_ERR_HIP, std::string(what) + ": " + hipGetErrorName(err) + " (" + hipGetErrorString(err) + ")");
}

// the checks an e4m3 cache adds, then the 16-bit launch's own
mfa_status prepare(const mfa_decode_params *p, const mfa_kv_quant *quant, Plan8 *plan) {
  if (!p || !quant) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (quant->cachePrecision == MFA_KV_E5M2)
    return fail(MFA_ERR_UNSUPPORTED, "an FP8 KV cache is e4m3 (MFA_KV_E4M3, OCP e4m3fn); e5m2 caches have no kernel");
  if (quant->cachePrecision != MFA_KV_E4M3)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_kv_quant.cachePrecision must be MFA_KV_E4M3 (16-bit caches: mfa_attention_decode_launch)");
  if (p->precision == MFA_FP32)
    return fail(MFA_ERR_UNSUPPORTED, "decode attention over an e4m3 cache takes a 16-bit Q (precision MFA_BF16 or MFA_FP16); FP32 Q has no kernel");
  static const char *names[2] = {"K", "V"};
  for (int i = 1; i <= 2; ++i) {
    bool ok = p->leadingDimension[i] % 16 == 0 && p->headStride[i] % 16 == 0;
    ok = ok && (p->pageSize ? p->pageStride[i - 1] % 16 == 0 : p->batchStride[i] % 16 == 0);
    if (!ok)
      return fail(MFA_ERR_INVALID_ARGUMENT, std::string("strides of ") + names[i - 1] +
                                                " must be multiples of 16 elements (16-byte rows of an e4m3 cache)");
  }
  const mfa_status st = decode_host_plan(p, &plan->host);
  if (st != MFA_OK) return st;
  plan->set = nullptr;
  for (const Decode8Set &s : kSets)
    if (s.D == p->headDimension && s.precision == p->precision) plan->set = &s;
  if (!plan->set) return fail(MFA_ERR_UNSUPPORTED, "decode attention is compiled for head dimensions 64 and 128");
  plan->keyScale = quant->keyScale;
  plan->valueScale = quant->valueScale;
  return MFA_OK;
}

mfa_status bind(Plan8 *plan, const void *q, const void *k, const void *v, void *o, float *l) {
  if (!q || !k || !v || !o) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if ((uintptr_t)q % 16 || (uintptr_t)k % 16 || (uintptr_t)v % 16 || (uintptr_t)o % 16)
    return fail(MFA_ERR_INVALID_ARGUMENT, "Q, K, V and O must be 16-byte aligned");
  if ((uintptr_t)l % 4) return fail(MFA_ERR_INVALID_ARGUMENT, "L must be 4-byte aligned");
  if ((uintptr_t)plan->keyScale % 4 || (uintptr_t)plan->valueScale % 4) return fail(MFA_ERR_INVALID_ARGUMENT, "keyScale and valueScale must be 4-byte aligned");
  DecodeArgs &a = plan->host.args;
  a.q = (const char *)q; a.k = (const char *)k; a.v = (const char *)v;
  a.o = (char *)o; a.l = l;
  return MFA_OK;
}

hipError_t run(const Plan8 &plan, hipStream_t stream) {
  const DecodeHostPlan &h = plan.host;
  hipError_t err;
  if (h.pieces > 1) {
    err = launch_kernel(plan.set->pieces, dim3(h.blocks * h.pieces), dim3(256), h.lds, stream, h.args, plan.keyScale, plan.valueScale);
    if (err != hipSuccess) return err;
    const uint64_t rows = (uint64_t)h.args.batches * h.args.Hq * h.args.R;
    err = launch_kernel(h.combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, stream, h.args);
  } else {
    err = launch_kernel(plan.set->single, dim3(h.blocks), dim3(256), h.lds, stream, h.args, plan.keyScale, plan.valueScale);
  }
  if (err != hipSuccess) return err;
  return hipGetLastError();
}

} // namespace

extern "C" {

void mfa_kv_quant_init(mfa_kv_quant *quant) {
  if (!quant) return;
  std::memset(quant, 0, sizeof(*quant));
  quant->cachePrecision = MFA_KV_E4M3;
}

mfa_status mfa_attention_decode_fp8_workspace_size(const mfa_decode_params *params, const mfa_kv_quant *quant, uint64_t *bytes) {
  if (!bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = 0;
  if (!params) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  mfa_decode_params probe = *params;   // the size does not depend on the workspace the caller may already have bound
  probe.workspace = nullptr;
  probe.workspaceBytes = 0;
  Plan8 plan;
  const mfa_status st = prepare(&probe, quant, &plan);
  if (st != MFA_OK) return st;
  if (plan.host.planned > 1) *bytes = decode_workspace_bytes(plan.host.planned, params);
  return MFA_OK;
}

mfa_status mfa_attention_decode_fp8_launch(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                           const mfa_kv_quant *quant, void *stream) {
  Plan8 plan;
  mfa_status st = prepare(params, quant, &plan);
  if (st != MFA_OK) return st;
  st = bind(&plan, q, k, v, o, l);
  if (st != MFA_OK) return st;
  const hipError_t err = run(plan, (hipStream_t)stream);
  if (err != hipSuccess) return hip_fail(err, plan.host.pieces > 1 ? plan.set->piecesName : plan.set->singleName);
  return MFA_OK;
}

mfa_status mfa_attention_decode_fp8_launch_form(const mfa_decode_params *params, const mfa_kv_quant *quant, char *out, size_t capacity) {
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  out[0] = '\0';
  Plan8 plan;
  const mfa_status st = prepare(params, quant, &plan);
  if (st != MFA_OK) return st;
  const DecodeHostPlan &h = plan.host;
  char text[512];
  const uint32_t M = h.args.G * h.args.R;
  if (h.pieces > 1)
    std::snprintf(text, sizeof(text), "%s (grid %u = %u sequences x K/V heads x %u pieces, %u packed rows, %s) + %s (grid %llu)",
                  plan.set->piecesName, h.blocks * h.pieces, h.blocks, h.pieces, M, h.args.paged ? "paged" : "contiguous", h.combineName,
                  (unsigned long long)(((uint64_t)h.args.batches * h.args.Hq * h.args.R + 3) / 4));
  else
    std::snprintf(text, sizeof(text), "%s (grid %u sequences x K/V heads, %u packed rows, %s%s)", plan.set->singleName, h.blocks, M,
                  h.args.paged ? "paged" : "contiguous",
                  h.planned > 1 ? (", unsplit without a workspace: the plan has " + std::to_string(h.planned) + " pieces").c_str() : "");
  std::strncpy(out, text, capacity - 1);
  out[capacity - 1] = '\0';
  return MFA_OK;
}

mfa_status mfa_attention_decode_fp8_time(const void *q, const void *k, const void *v, void *o, float *l, const mfa_decode_params *params,
                                         const mfa_kv_quant *quant, void *stream, int warmup, int iterations, float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  Plan8 plan;
  mfa_status st = prepare(params, quant, &plan);
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
