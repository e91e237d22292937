// kv_e4m3.h -- the e4m3 (OCP e4m3fn) codec of the FP8 KV cache: ONE body for the exported host functions (mfa_kv_quantize_e4m3 /
// mfa_kv_dequantize_e4m3, include/mfa_kvcache.h) and for the append kernel, so that the writer, the reader and the tests agree on
// rounding, saturation and the scale convention by construction.  Integer arithmetic but for the IEEE division and one FP32 add.
//
// cvt8_e4m3 is what the attention kernels read the cache with (attn_decode16.h, attn_prefill16.h): the hardware's conversion to the
// launch's 16-bit type, exact (e4m3 has 3 mantissa bits and a range of 2^-9 .. 448), so it agrees with kv_dequantize_e4m3 bit for bit.
#pragma once
#include "attn_common.h"

namespace mfa {

// round-to-nearest-even e4m3 of clamp(x / scale, -448, 448); NaN -> 0x7f | sign; -0 kept
__host__ __device__ __forceinline__ uint8_t kv_quantize_e4m3(float x, float scale) {
  const float y = x / scale;
  const uint32_t bits = __builtin_bit_cast(uint32_t, y);
  const uint32_t sign = (bits >> 24) & 0x80u, a = bits & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint8_t)(sign | 0x7Fu);          // NaN
  if (a >= 0x43E00000u) return (uint8_t)(sign | 0x7Eu);         // |y| >= 448 (infinity included): saturate
  if (a >= 0x3C800000u) {                                       // |y| >= 2^-6: a normal e4m3; 23 -> 3 mantissa bits, ties to even
    const uint32_t r = (a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20; // (exponent << 3 | mantissa), a carry moves to the exponent
    return (uint8_t)(sign | (r - (120u << 3)));                 // bias 127 -> 7
  }
  // subnormal: multiples of 2^-9.  |y| 2^9 is exact; adding 1.5 2^23 rounds it to an integer, ties to even, in the low mantissa bits
  const float t = __builtin_bit_cast(float, a) * 512.0f + 12582912.0f;
  return (uint8_t)(sign | (__builtin_bit_cast(uint32_t, t) & 0xFu));   // 0 .. 8 (8 = the smallest normal)
}

__host__ __device__ __forceinline__ float kv_dequantize_e4m3(uint8_t byte) {
  const uint32_t sign = (uint32_t)(byte & 0x80u) << 24, e = (byte >> 3) & 15u, m = byte & 7u;
  if ((byte & 0x7Fu) == 0x7Fu) return __builtin_bit_cast(float, sign | 0x7FC00000u);
  if (e == 0) return __builtin_bit_cast(float, sign | __builtin_bit_cast(uint32_t, (float)m * 0.001953125f));
  return __builtin_bit_cast(float, sign | ((e + 120u) << 23) | (m << 20));
}

// eight e4m3 bytes (two dwords) -> eight values of the 16-bit type T, in order (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0)
template <typename T> __device__ __forceinline__ u32x4 cvt8_e4m3(uint32_t lo, uint32_t hi) {
  if constexpr (__is_same(T, __bf16)) {
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true))};
  } else {
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true))};
  }
}

} // namespace mfa
