// kv_latent_append.hip -- appends the R new rows of every sequence to the LATENT cache of multi-head latent attention
// (include/mfa_mla_cache.h): one cache row of 576 elements per key, 512 from latentNew and 64 from ropeNew.  An elementwise kernel after
// kv_cache_append.hip: a thread moves 8 source elements -- one 16-byte load, then an 8-byte store into an e4m3 cache (quantised by
// kv_quantize_e4m3, the exported contract, with the cache's ONE scale) or a 16-byte store into a 16-bit cache (bits copied).  A row has
// 72 such chunks, 64 latent and 8 rotary; the threads of the launch are the chunks of all batches x R rows, flat, so no lane idles
// on a row of 72 and `rows` has no limit.  Where a row goes, and which rows are dropped, is kv_cache_slot()'s to say.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>

#include "../../include/mfa_mla_cache.h"
#include "attn_common.h"
#include "cache_launch.h"
#include "kv_cache_slot.h"
#include "kv_e4m3.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

namespace {

constexpr uint32_t LATENT = MFA_MLA_LATENT_DIMENSION, ROPE = MFA_MLA_ROPE_DIMENSION;
constexpr uint32_t LATENT_CHUNKS = LATENT / 8, ROW_CHUNKS = (LATENT + ROPE) / 8;   // 64 of the 72 chunks of a row are latent

struct LatentAppendArgs {
  const char *src[2];             // latentNew, ropeNew
  char *dst;
  const float *scale;             // one entry; null: 1.0
  const uint32_t *lengths;
  const int32_t *table;
  int64_t tableStride;
  int64_t lds[2], bss[2];         // sources; elements
  int64_t ldc, bsc, psc;
  uint32_t R, batches, column;
  uint32_t paged, pageShift;
};

template <typename T> __device__ __forceinline__ float to_float(uint16_t bits);
template <> __device__ __forceinline__ float to_float<__bf16>(uint16_t bits) { return __builtin_bit_cast(float, (uint32_t)bits << 16); }
template <> __device__ __forceinline__ float to_float<_Float16>(uint16_t bits) { return (float)__builtin_bit_cast(_Float16, bits); }

template <typename T, bool FP8>
__device__ __forceinline__ void latent_append_body(const LatentAppendArgs &a) {
  const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t rowid = item / ROW_CHUNKS;
  const uint32_t c = (uint32_t)(item % ROW_CHUNKS);
  if (rowid >= (uint64_t)a.batches * a.R) return;
  const uint32_t batch = (uint32_t)(rowid / a.R), row = (uint32_t)(rowid % a.R);
  int64_t outer, in;
  if (!kv_cache_slot(a.table, a.tableStride, a.paged, a.pageShift, a.column, batch, (int64_t)a.lengths[batch] - (int64_t)a.R + (int64_t)row,
                     &outer, &in))
    return;
  const int o = c >= LATENT_CHUNKS;   // 0: a latent chunk, 1: a rotary one
  const uint32_t sc = o ? c - LATENT_CHUNKS : c;
  const u32x4 x = *reinterpret_cast<const u32x4 *>(a.src[o] + ((int64_t)batch * a.bss[o] + (int64_t)row * a.lds[o] + 8 * sc) * 2);
  const int64_t at = outer * (a.paged ? a.psc : a.bsc) + in * a.ldc + 8 * c;   // (the rotary part follows the latent: 8 c from the row)
  if constexpr (FP8) {
    const float scale = a.scale ? a.scale[0] : 1.0f;
    u32x2 out = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint16_t bits = (uint16_t)(x[i >> 1] >> (16 * (i & 1)));
      out[i >> 2] |= (uint32_t)kv_quantize_e4m3(to_float<T>(bits), scale) << (8 * (i & 3));
    }
    *reinterpret_cast<u32x2 *>(a.dst + at) = out;
  } else {
    *reinterpret_cast<u32x4 *>(a.dst + at * 2) = x;
  }
}

} // namespace

extern "C" __global__ __launch_bounds__(256) void kv_latent_append_bf16_e4m3(const LatentAppendArgs a) { latent_append_body<__bf16, true>(a); }
extern "C" __global__ __launch_bounds__(256) void kv_latent_append_f16_e4m3(const LatentAppendArgs a) { latent_append_body<_Float16, true>(a); }
// a 16-bit cache takes the bits as they are: one kernel serves both types
extern "C" __global__ __launch_bounds__(256) void kv_latent_append_copy16(const LatentAppendArgs a) { latent_append_body<__bf16, false>(a); }

namespace {

typedef CacheKernel<LatentAppendArgs> LatentAppendKernel;
const LatentAppendKernel kKernels[3] = {MFA_CACHE_KERNEL(kv_latent_append_copy16), MFA_CACHE_KERNEL(kv_latent_append_bf16_e4m3),
                                        MFA_CACHE_KERNEL(kv_latent_append_f16_e4m3)};   // a 16-bit cache, bf16 rows into e4m3, f16 rows into e4m3

// every check that needs no GPU, and the kernel's argument block (the buffer pointers are filled in by the entry)
mfa_status prepare(const mfa_mla_append_params *p, LatentAppendArgs *a, const LatentAppendKernel **kernel, uint32_t *grid) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->precision != MFA_BF16 && p->precision != MFA_FP16)
    return fail(p->precision == MFA_FP32 ? MFA_ERR_UNSUPPORTED : MFA_ERR_INVALID_ARGUMENT,
                "the new latent / rotary rows must be 16-bit (precision MFA_FP16 or MFA_BF16)");
  bool fp8;
  mfa_status st = check_cache_precision(p->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8 && p->cachePrecision != p->precision)
    return fail(MFA_ERR_INVALID_ARGUMENT, "cachePrecision must be the rows' 16-bit type (`precision`) or MFA_KV_E4M3");
  if (p->latentDimension != LATENT || p->ropeDimension != ROPE)
    return fail(MFA_ERR_UNSUPPORTED, "the latent cache append is compiled for (latentDimension, ropeDimension) = (512, 64), not (" +
                                         std::to_string(p->latentDimension) + ", " + std::to_string(p->ropeDimension) + ")");
  if (p->rows == 0 || p->batches == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "rows and batches must be non-zero");
  const uint64_t blocks = ((uint64_t)p->rows * p->batches * ROW_CHUNKS + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "rows x batches x 72 chunks must fit a grid of 2^31 - 1 workgroups of 256");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  if (!fp8 && p->kvScale)
    return fail(MFA_ERR_INVALID_ARGUMENT, "kvScale goes with an e4m3 cache (MFA_KV_E4M3); a 16-bit cache takes the rows' bits unscaled");
  uint32_t pageShift = 0;
  st = check_written_cache(p->pageSize, p->blockTable, p->blockTableStride, p->column, &pageShift);
  if (st != MFA_OK) return st;
  st = check_operand_strides("latentNew", LATENT, p->leadingDimension[0], 0, p->batchStride[0], 8, kWrittenCacheStridesWhy);
  if (st == MFA_OK) st = check_operand_strides("ropeNew", ROPE, p->leadingDimension[1], 0, p->batchStride[1], 8, kWrittenCacheStridesWhy);
  if (st == MFA_OK)
    st = check_written_cache_strides("kvCache", LATENT + ROPE, p->leadingDimension[2], 0, p->pageSize ? p->pageStride : p->batchStride[2], fp8);
  if (st != MFA_OK) return st;
  std::memset(a, 0, sizeof(*a));
  a->scale = p->kvScale;
  a->lengths = p->cacheLengths;
  a->table = p->blockTable;
  a->tableStride = p->blockTableStride;
  for (int o = 0; o < 2; ++o) a->lds[o] = p->leadingDimension[o], a->bss[o] = p->batchStride[o];
  a->ldc = p->leadingDimension[2]; a->bsc = p->batchStride[2]; a->psc = p->pageStride;
  a->R = p->rows; a->batches = p->batches; a->column = p->column;
  a->paged = p->pageSize != 0; a->pageShift = pageShift;
  *kernel = &kKernels[!fp8 ? 0 : p->precision == MFA_BF16 ? 1 : 2];
  *grid = (uint32_t)blocks;
  return MFA_OK;
}

} // namespace

extern "C" {

void mfa_mla_append_params_init(mfa_mla_append_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->precision = params->cachePrecision = MFA_BF16;
  params->latentDimension = MFA_MLA_LATENT_DIMENSION;
  params->ropeDimension = MFA_MLA_ROPE_DIMENSION;
}

size_t mfa_mla_append_params_size(void) { return sizeof(mfa_mla_append_params); }

mfa_status mfa_mla_append_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_AT(FIELD) (uint32_t)offsetof(mfa_mla_append_params, FIELD)
  static const uint32_t table[] = {MFA_AT(rows), MFA_AT(batches), MFA_AT(column), MFA_AT(pageSize), MFA_AT(latentDimension), MFA_AT(ropeDimension),
                                   MFA_AT(precision), MFA_AT(cachePrecision), MFA_AT(reserved), MFA_AT(cacheLengths), MFA_AT(blockTable),
                                   MFA_AT(blockTableStride), MFA_AT(leadingDimension), MFA_AT(batchStride), MFA_AT(pageStride), MFA_AT(kvScale)};
#undef MFA_AT
  const uint32_t fields = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = fields;
  for (uint32_t i = 0; i < fields && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_mla_cache_append_launch(const void *latentNew, const void *ropeNew, void *kvCache, const mfa_mla_append_params *params,
                                       void *stream) {
  LatentAppendArgs a;
  const LatentAppendKernel *kernel = nullptr;
  uint32_t grid = 0;
  mfa_status st = prepare(params, &a, &kernel, &grid);
  if (st == MFA_OK) st = check_buffers({latentNew, ropeNew, kvCache}, "latentNew, ropeNew and kvCache");
  if (st == MFA_OK) st = check_float_arrays({a.scale}, "kvScale");
  if (st != MFA_OK) return st;
  a.src[0] = (const char *)latentNew; a.src[1] = (const char *)ropeNew;
  a.dst = (char *)kvCache;
  hipError_t err = launch_kernel(kernel->launch, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  if (err == hipSuccess) err = hipGetLastError();
  if (err != hipSuccess) return hip_fail(err, kernel->name);
  return MFA_OK;
}

} // extern "C"
