// kv_cache_append.hip -- appends the R new key / value rows of every sequence to a KV cache (include/mfa_kvcache.h): an elementwise
// kernel; 16-byte loads of the 16-bit source rows, 8-byte stores into an e4m3 cache (quantised by kv_quantize_e4m3, the exported
// contract) or 16-byte stores into a 16-bit cache (bits copied).  One workgroup per (sequence, new row): the row's position and, for a
// paged cache, its one block-table entry are workgroup-uniform.  The ragged launch (include/mfa_ragged.h: packed sources, one workgroup
// per packed row, which finds its sequence by an upper-bound search in rowStarts) runs the same store path.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/mfa_kvcache.h"
#include "../../include/mfa_ragged.h"
#include "attn_common.h"
#include "cache_launch.h"
#include "kv_cache_slot.h"
#include "kv_e4m3.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

namespace {

struct AppendArgs {
  const char *src[2];             // kNew, vNew
  char *dst[2];                   // kCache, vCache
  const float *scale[2];
  const uint32_t *lengths;
  const int32_t *table;
  int64_t tableStride;
  int64_t lds[2], hss[2], bss[2]; // sources; elements
  int64_t ldc[2], hsc[2], bsc[2], psc[2];
  uint32_t R, H, column;
  uint32_t paged, pageShift;
  const uint32_t *rowStarts;      // the ragged kernels only: [batches + 1]; last, so that no other field moves
  uint32_t totalRows, batches;
};

template <typename T> __device__ __forceinline__ float to_float(uint16_t bits);
template <> __device__ __forceinline__ float to_float<__bf16>(uint16_t bits) { return __builtin_bit_cast(float, (uint32_t)bits << 16); }
template <> __device__ __forceinline__ float to_float<_Float16>(uint16_t bits) { return (float)__builtin_bit_cast(_Float16, bits); }

// the workgroup's row: source row `row` of source batch `sbatch` goes to key `pos` of sequence `batch`
template <typename T, int D, bool FP8>
__device__ __forceinline__ void kv_append_row(const AppendArgs &a, uint32_t batch, uint32_t sbatch, uint32_t row, int64_t pos) {
  constexpr uint32_t CPR = D / 8;   // 16-byte source chunks per row
  int64_t base[2], outer, in;
  if (!kv_cache_slot(a.table, a.tableStride, a.paged, a.pageShift, a.column, batch, pos, &outer, &in)) return;
#pragma unroll
  for (int o = 0; o < 2; ++o) base[o] = outer * (a.paged ? a.psc[o] : a.bsc[o]) + in * a.ldc[o];
  const uint32_t items = 2u * a.H * CPR;
  for (uint32_t idx = threadIdx.x; idx < items; idx += blockDim.x) {
    const uint32_t c = idx % CPR, head = (idx / CPR) % a.H, o = idx / (CPR * a.H);
    const char *sp = a.src[o] + ((int64_t)sbatch * a.bss[o] + (int64_t)head * a.hss[o] + (int64_t)row * a.lds[o] + 8 * c) * 2;
    const u32x4 x = *reinterpret_cast<const u32x4 *>(sp);
    const int64_t at = base[o] + (int64_t)head * a.hsc[o] + 8 * c;
    if constexpr (FP8) {
      const float scale = a.scale[o] ? a.scale[o][head] : 1.0f;
      u32x2 out = {0u, 0u};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint16_t bits = (uint16_t)(x[i >> 1] >> (16 * (i & 1)));
        out[i >> 2] |= (uint32_t)kv_quantize_e4m3(to_float<T>(bits), scale) << (8 * (i & 3));
      }
      *reinterpret_cast<u32x2 *>(a.dst[o] + at) = out;
    } else {
      *reinterpret_cast<u32x4 *>(a.dst[o] + at * 2) = x;
    }
  }
}

template <typename T, int D, bool FP8>
__device__ __forceinline__ void kv_append_body(const AppendArgs &a) {
  const uint32_t batch = blockIdx.x / a.R, row = blockIdx.x % a.R;
  kv_append_row<T, D, FP8>(a, batch, batch, row, (int64_t)a.lengths[batch] - (int64_t)a.R + (int64_t)row);
}

// RAGGED: workgroup t owns packed row t < T.  Its sequence is the last b with rowStarts[b] <= t (an upper-bound search over
// rowStarts[0 .. batches), which stays inside the array whatever it holds); with s_b, qn_b of include/mfa_ragged.h the row is r = t - s_b
// when r < qn_b, and belongs to nobody otherwise (past the cap `R`, or starts that decrease).
template <typename T, int D, bool FP8>
__device__ __forceinline__ void kv_append_ragged_body(const AppendArgs &a) {
  const uint32_t t = blockIdx.x;
  uint32_t lo = 0, hi = a.batches;   // the first b in [0, batches] with rowStarts[b] > t, taking rowStarts[batches] as past everything
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.rowStarts[mid] <= t) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const uint32_t batch = lo - 1, T_ = a.totalRows;
  const uint32_t s0 = a.rowStarts[batch], e0 = a.rowStarts[batch + 1];
  const uint32_t s = s0 < T_ ? s0 : T_, e = e0 < T_ ? e0 : T_;
  const uint32_t span = e > s ? e - s : 0u, qn = span < a.R ? span : a.R, r = t - s;
  if (r >= qn) return;
  kv_append_row<T, D, FP8>(a, batch, 0u, t, (int64_t)a.lengths[batch] - (int64_t)qn + (int64_t)r);
}

} // namespace

#define MFA_KV_APPEND_KERNELS(TN, T, D)                                                                                               \
  extern "C" __global__ __launch_bounds__(256) void kv_cache_append_d##D##_##TN##_e4m3(const AppendArgs a) {                          \
    kv_append_body<T, D, true>(a);                                                                                                    \
  }                                                                                                                                   \
  extern "C" __global__ __launch_bounds__(256) void kv_cache_append_ragged_d##D##_##TN##_e4m3(const AppendArgs a) {                   \
    kv_append_ragged_body<T, D, true>(a);                                                                                             \
  }
MFA_KV_APPEND_KERNELS(bf16, __bf16, 64)
MFA_KV_APPEND_KERNELS(bf16, __bf16, 128)
MFA_KV_APPEND_KERNELS(bf16, __bf16, 256)
MFA_KV_APPEND_KERNELS(f16, _Float16, 64)
MFA_KV_APPEND_KERNELS(f16, _Float16, 128)
MFA_KV_APPEND_KERNELS(f16, _Float16, 256)
// a 16-bit cache takes the bits as they are: one kernel per head dimension serves both types
#define MFA_KV_COPY_KERNELS(D)                                                                                                        \
  extern "C" __global__ __launch_bounds__(256) void kv_cache_append_d##D##_copy16(const AppendArgs a) { kv_append_body<__bf16, D, false>(a); } \
  extern "C" __global__ __launch_bounds__(256) void kv_cache_append_ragged_d##D##_copy16(const AppendArgs a) {                        \
    kv_append_ragged_body<__bf16, D, false>(a);                                                                                       \
  }
MFA_KV_COPY_KERNELS(64)
MFA_KV_COPY_KERNELS(128)
MFA_KV_COPY_KERNELS(256)

namespace {

typedef void (*AppendKernel)(const AppendArgs);
struct AppendEntry {
  AppendKernel launch;
  const char *name;
};
struct AppendSet {
  uint32_t D;
  AppendEntry kernel[2][3];   // [ragged][0: a 16-bit cache, 1: bf16 rows into e4m3, 2: f16 rows into e4m3]
};
#define MFA_KV_APPEND_ENTRY(NAME) {NAME, #NAME}
#define MFA_KV_APPEND_SET(D)                                                                                                          \
  {D,                                                                                                                                 \
   {{MFA_KV_APPEND_ENTRY(kv_cache_append_d##D##_copy16), MFA_KV_APPEND_ENTRY(kv_cache_append_d##D##_bf16_e4m3),                       \
     MFA_KV_APPEND_ENTRY(kv_cache_append_d##D##_f16_e4m3)},                                                                           \
    {MFA_KV_APPEND_ENTRY(kv_cache_append_ragged_d##D##_copy16), MFA_KV_APPEND_ENTRY(kv_cache_append_ragged_d##D##_bf16_e4m3),         \
     MFA_KV_APPEND_ENTRY(kv_cache_append_ragged_d##D##_f16_e4m3)}}}
const AppendSet kSets[] = {MFA_KV_APPEND_SET(64), MFA_KV_APPEND_SET(128), MFA_KV_APPEND_SET(256)};

mfa_status prepare(const mfa_kv_append_params *p, AppendArgs *a, AppendKernel *kernel, const char **name, const mfa_ragged_rows *ragged) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (ragged) {
    if (!ragged->rowStarts)
      return fail(MFA_ERR_INVALID_ARGUMENT, "rowStarts is required (device array of batches + 1 uint32: the first packed row of every sequence, and the end of the last)");
    if (ragged->totalRows == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "totalRows must be non-zero (the packed rows of kNew and vNew)");
    if (ragged->totalRows > 0x7FFFFFFFu) return fail(MFA_ERR_INVALID_ARGUMENT, "totalRows must fit a grid of 2^31 - 1 workgroups");
    if (p->batchStride[0] != 0 || p->batchStride[1] != 0)
      return fail(MFA_ERR_INVALID_ARGUMENT, "batchStride of kNew and vNew must be 0 for a ragged launch: the packed layout [totalRows][heads][D] has no batch axis");
  }
  if (p->precision != MFA_BF16 && p->precision != MFA_FP16)
    return fail(p->precision == MFA_FP32 ? MFA_ERR_UNSUPPORTED : MFA_ERR_INVALID_ARGUMENT,
                "the new key / value rows must be 16-bit (precision MFA_FP16 or MFA_BF16)");
  bool fp8;
  mfa_status st = check_cache_precision(p->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8 && p->cachePrecision != p->precision)
    return fail(MFA_ERR_INVALID_ARGUMENT, "cachePrecision must be the rows' 16-bit type (`precision`) or MFA_KV_E4M3");
  const AppendSet *set = nullptr;
  for (const AppendSet &s : kSets)
    if (s.D == p->headDimension) set = &s;
  if (!set)
    return fail(MFA_ERR_UNSUPPORTED, "the KV cache append is compiled for head dimensions 256, 64 and 128, not " + std::to_string(p->headDimension));
  if (p->rows == 0 || p->heads == 0 || p->batches == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "rows, heads and batches must be non-zero");
  if (!ragged && (uint64_t)p->rows * p->batches > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "rows x batches must fit a grid of 2^31 - 1 workgroups");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  if (!fp8 && (p->keyScale || p->valueScale))
    return fail(MFA_ERR_INVALID_ARGUMENT, "keyScale / valueScale go with an e4m3 cache (MFA_KV_E4M3); a 16-bit cache takes the rows' bits unscaled");
  uint32_t pageShift = 0;
  st = check_written_cache(p->pageSize, p->blockTable, p->blockTableStride, p->column, &pageShift);
  if (st != MFA_OK) return st;
  static const char *names[4] = {"kNew", "vNew", "kCache", "vCache"};
  for (int i = 0; i < 4; ++i) {
    if (i >= 2)
      st = check_written_cache_strides(names[i], p->headDimension, p->leadingDimension[i], p->headStride[i],
                                       p->pageSize ? p->pageStride[i - 2] : p->batchStride[i], fp8);
    else
      st = check_operand_strides(names[i], p->headDimension, p->leadingDimension[i], p->headStride[i], p->batchStride[i], 8, kWrittenCacheStridesWhy);
    if (st != MFA_OK) return st;
  }
  std::memset(a, 0, sizeof(*a));
  a->scale[0] = p->keyScale; a->scale[1] = p->valueScale;
  a->lengths = p->cacheLengths;
  a->table = p->blockTable;
  a->tableStride = p->blockTableStride;
  for (int o = 0; o < 2; ++o) {
    a->lds[o] = p->leadingDimension[o]; a->hss[o] = p->headStride[o]; a->bss[o] = p->batchStride[o];
    a->ldc[o] = p->leadingDimension[2 + o]; a->hsc[o] = p->headStride[2 + o]; a->bsc[o] = p->batchStride[2 + o];
    a->psc[o] = p->pageStride[o];
  }
  a->R = p->rows; a->H = p->heads; a->column = p->column;
  a->paged = p->pageSize != 0; a->pageShift = pageShift;
  if (ragged) {
    a->rowStarts = ragged->rowStarts; a->totalRows = ragged->totalRows; a->batches = p->batches;
  }
  const AppendEntry &entry = set->kernel[ragged != nullptr][!fp8 ? 0 : p->precision == MFA_BF16 ? 1 : 2];
  *kernel = entry.launch;
  *name = entry.name;
  return MFA_OK;
}

} // namespace

extern "C" {

uint8_t mfa_kv_quantize_e4m3(float x, float scale) { return kv_quantize_e4m3(x, scale); }
float mfa_kv_dequantize_e4m3(uint8_t byte) { return kv_dequantize_e4m3(byte); }

void mfa_kv_append_params_init(mfa_kv_append_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->cachePrecision = MFA_BF16;
}

static mfa_status append_launch(const void *kNew, const void *vNew, void *kCache, void *vCache, const mfa_kv_append_params *params,
                                const mfa_ragged_rows *ragged, void *stream) {
  AppendArgs a;
  AppendKernel kernel = nullptr;
  const char *name = "";
  mfa_status st = prepare(params, &a, &kernel, &name, ragged);
  if (st == MFA_OK) st = check_buffers({kNew, vNew, kCache, vCache}, "kNew, vNew, kCache and vCache");
  if (st != MFA_OK) return st;
  a.src[0] = (const char *)kNew; a.src[1] = (const char *)vNew;
  a.dst[0] = (char *)kCache; a.dst[1] = (char *)vCache;
  hipError_t err = launch_kernel(kernel, dim3(ragged ? ragged->totalRows : params->batches * params->rows), dim3(256), 0, (hipStream_t)stream, a);
  if (err == hipSuccess) err = hipGetLastError();
  if (err != hipSuccess) return hip_fail(err, name);
  return MFA_OK;
}

mfa_status mfa_kv_cache_append_launch(const void *kNew, const void *vNew, void *kCache, void *vCache, const mfa_kv_append_params *params,
                                      void *stream) {
  return append_launch(kNew, vNew, kCache, vCache, params, nullptr, stream);
}

mfa_status mfa_kv_cache_append_ragged_launch(const void *kNew, const void *vNew, void *kCache, void *vCache, const mfa_kv_append_params *params,
                                             const mfa_ragged_rows *ragged, void *stream) {
  if (!ragged)
    return fail(MFA_ERR_INVALID_ARGUMENT, "null mfa_ragged_rows: the ragged append requires the block (mfa_ragged_rows_init; one row count "
                                          "for every sequence: mfa_kv_cache_append_launch)");
  return append_launch(kNew, vNew, kCache, vCache, params, ragged, stream);
}

} // extern "C"
