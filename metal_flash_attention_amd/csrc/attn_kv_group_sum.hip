// attn_kv_group_sum.hip -- dK / dV of grouped-query attention (mfa_launch_params.headsPerKeyValue = G > 1).
//
// The backwardKeyValue kernels run over the Hq query heads and leave each head's fp32 dK / dV in a slab of the caller's workspace,
// [batch][query head][column][D] (prepare_launch, mfa_kernel.hip).  This kernel adds, for K / V head j, the G slabs of query heads
// jG .. jG + G - 1 in that order in fp32 (no atomics: every output element has one lane) and stores the sum through the caller's dK /
// dV view in its precision (BF16 by truncation, FP16 round-to-nearest, FP32), leading dimension and strides; batch entry b stores only
// its columns < columnLengths[b].  HBM-bound: 2 x Hq x column x D x 4 bytes read, the outputs written once.
#include "launchers.h"

namespace mfa {

// V = 8: eight consecutive elements of one row per lane, two 16-byte loads per slab, all slabs of a batch of 8 in flight together,
// one 16-byte store (16-bit outputs) or two (FP32).  V = 1: one element per lane, any D / alignment; transposed outputs ([D][column])
// walk the columns fastest so that neighbouring lanes store neighbouring elements.
// grid = (2 x blocks: dV then dK, K / V heads, batches); 256 lanes per workgroup, one chunk of V elements each.
template <int V>
static __global__ __launch_bounds__(256) void attn_kv_group_sum(const float *dvSlabs, const float *dkSlabs, OperandView dv, OperandView dk,
                                                                uint32_t G, uint32_t C, uint32_t D, uint32_t blocks, const uint32_t *colLen) {
  const bool isK = blockIdx.x >= blocks;
  const uint32_t blk = isK ? blockIdx.x - blocks : blockIdx.x;
  const uint32_t j = blockIdx.y, b = blockIdx.z, Hq = gridDim.y * G;
  const uint32_t e = blk * 256 + threadIdx.x;   // chunk of this (head, batch) slice
  const uint32_t chunksPerRow = D / V;
  if (e >= C * chunksPerRow) return;
  char *optr = static_cast<char *>(isK ? dk.ptr : dv.ptr);
  const int64_t ld = isK ? dk.ld : dv.ld, hs = isK ? dk.headStride : dv.headStride, bs = isK ? dk.batchStride : dv.batchStride;
  const int prec = isK ? dk.precision : dv.precision;
  const bool tr = V == 1 && (isK ? dk.transposed : dv.transposed);
  uint32_t c, d;
  if (tr) { c = e % C; d = e / C; }
  else { c = e / chunksPerRow; d = (e % chunksPerRow) * V; }
  if (colLen && c >= colLen[b]) return;   // padding of the batch entry: neither read nor written

  const uint64_t gstride = (uint64_t)C * D;
  const float *src = (isK ? dkSlabs : dvSlabs) + ((uint64_t)b * Hq + (uint64_t)j * G) * gstride + (uint64_t)c * D + d;
  float acc[V];
  auto load = [&](const float *p, float *x) {
    if constexpr (V == 8) {
      const float4 lo = reinterpret_cast<const float4 *>(p)[0], hi = reinterpret_cast<const float4 *>(p)[1];
      x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
    } else {
      x[0] = p[0];
    }
  };
  load(src, acc);
  for (uint32_t g0 = 1; g0 < G; g0 += 8) {   // (G is uniform: the guards are scalar branches, the loads of a batch issue back to back)
    float x[8][V];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (g0 + k < G) load(src + (g0 + k) * gstride, x[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (g0 + k < G) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += x[k][v];
      }
  }

  char *base = optr + ((int64_t)j * hs + (int64_t)b * bs) * (prec == PREC_FP32 ? 4 : 2);
  if constexpr (V == 8) {
    const int64_t off = (int64_t)c * ld + d;
    if (prec == PREC_FP32) {
      float4 *o = reinterpret_cast<float4 *>(reinterpret_cast<float *>(base) + off);
      o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else if (prec == PREC_FP16) {
      f16x8 h;
#pragma unroll
      for (int v = 0; v < 8; ++v) h[v] = (_Float16)acc[v];
      *reinterpret_cast<f16x8 *>(reinterpret_cast<_Float16 *>(base) + off) = h;
    } else {
      u32x4 h;
#pragma unroll
      for (int v = 0; v < 4; ++v) h[v] = (uint32_t)f32_to_bf16_trunc(acc[2 * v]) | ((uint32_t)f32_to_bf16_trunc(acc[2 * v + 1]) << 16);
      *reinterpret_cast<u32x4 *>(reinterpret_cast<uint16_t *>(base) + off) = h;
    }
  } else {
    store_elem(base, tr ? (int64_t)d * ld + c : (int64_t)c * ld + d, prec, acc[0]);
  }
}

// the 16-byte path: whole 8-element chunks in rows whose every start is 16-byte aligned, row-major
static bool wide_output(const OperandView &v, uint32_t D) {
  const int64_t per16 = v.precision == PREC_FP32 ? 4 : 8;
  return !v.transposed && (D % 8) == 0 && (reinterpret_cast<uintptr_t>(v.ptr) & 15) == 0 && v.ld % per16 == 0 && v.headStride % per16 == 0 &&
         v.batchStride % per16 == 0;
}

hipError_t launch_kv_group_sum(const float *dvSlabs, const float *dkSlabs, const OperandView &dv, const OperandView &dk, uint32_t G,
                               uint32_t kvHeads, uint32_t batches, uint32_t C, uint32_t D, const uint32_t *colLen, hipStream_t stream) {
  const bool wide = wide_output(dv, D) && wide_output(dk, D);
  const uint64_t chunks = (uint64_t)C * (wide ? D / 8 : D);
  if (chunks > 0xFFFFFFFFull - 255) return hipErrorInvalidValue;   // (a slice of more than 2^32 chunks: prepare_launch refuses it)
  const uint32_t blocks = (uint32_t)((chunks + 255) / 256);
  const dim3 grid(2 * blocks, kvHeads, batches);
  if (wide) return launch_kernel(&attn_kv_group_sum<8>, grid, dim3(256), 0, stream, dvSlabs, dkSlabs, dv, dk, G, C, D, blocks, colLen);
  return launch_kernel(&attn_kv_group_sum<1>, grid, dim3(256), 0, stream, dvSlabs, dkSlabs, dv, dk, G, C, D, blocks, colLen);
}

} // namespace mfa
