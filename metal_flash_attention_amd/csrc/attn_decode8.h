// attn_decode8.h -- decode attention over an FP8 (OCP e4m3) KV cache (include/mfa_kvcache.h): the kernel of
// attn_decode16.h with K and V read as bytes.  What is the same: one workgroup per K / V head of a sequence (and piece), the G R
// packed query rows, four waves walking their own 32-key steps without a barrier, the fragment maps, the masking and poison rules, the
// LDS merge of the waves, decode_piece_range, the workspace slabs and the combine kernel.  What differs:
//   * Q stays 16-bit; K and V bytes are CONVERTED in registers to the launch's 16-bit type (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale
//     1.0: exact, e4m3 has 3 mantissa bits and a range of 2^-9 .. 448) and feed the same v_mfma_f32_32x32x16.  The FP8 matrix
//     instruction is not used: the kernel is bound by bytes, not by the matrix pipe.
//   * K: a lane is still a key row, but a 16-byte load now spans 16 values of d.  The loads stay 16 bytes wide (half as many per step)
//     and the contraction index is permuted instead: matrix step 2u + v of the lane half `hi` contracts d = 32 u + 16 hi + 8 v .. + 7,
//     the bytes 8 v .. 8 v + 7 of load u, and the Q fragments are loaded with the same permutation.  The raw bytes wait in registers;
//     a slice is converted at its matrix instruction.
//   * V: 16-byte loads of whole rows (half as many per step), converted before the LDS write, so that the wave's V image
//     [D/32][32 keys][32 d] and the ds_read_b64_tr_b16 gather are those of the 16-bit kernel.
//   * the scales are per K / V head: keyScale folds into the softmax scale, valueScale into the final normalisation (pieces: into
//     the un-normalised O they publish, so that the combine kernel needs no change).
//   * poison: rows at or past the piece's end are not loaded (zero bytes = +0.0), so a 0x7f beyond a length never reaches a product.
#pragma once
#include "attn_decode16.h"

namespace mfa {

// eight e4m3 bytes (two dwords) -> eight values of the 16-bit type T, in order
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

template <typename T, int D, bool SPLIT>
__device__ __forceinline__ void decode8_body(const DecodeArgs &a, const float *keyScale, const float *valueScale) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NDB = D / 32, NKS = D / 16, NKL = D / 32;   // matrix steps along d; 16-byte K loads per lane
  constexpr int CPR = D / 16;                  // 16-byte chunks per row (16 values of d)
  constexpr int RPI = 64 / CPR;                // V rows one wave-instruction covers
  constexpr int NCH = DEC_STEP / RPI;          // V chunks per lane per step
  constexpr int IMAGE = DEC_STEP * D * 2;      // bytes of a wave's V image (16-bit values)
  static_assert(16 % RPI == 0, "a lane's V rows of one instruction stay inside a 16-key group");

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t piece = SPLIT ? blockIdx.x % a.pieces : 0u;
  const uint32_t hb = SPLIT ? blockIdx.x / a.pieces : blockIdx.x;
  const uint32_t kvh = hb % a.Hkv, batch = hb / a.Hkv;
  const uint32_t R = a.R, M = a.G * R;
  const uint32_t len = min(a.lengths[batch], a.column);
  uint32_t begin = 0, end = len;
  if constexpr (SPLIT) decode_piece_range(len, a.pieces, piece, &begin, &end);
  const float kscale = a.scale2 * (keyScale ? keyScale[kvh] : 1.0f);
  const float vscale = valueScale ? valueScale[kvh] : 1.0f;

  // ---- the lane's packed query row (attn_decode16.h), its fragments in the permuted contraction order of the K bytes
  const uint32_t pc = min((uint32_t)q, M - 1);
  const uint32_t qhead = kvh * a.G + pc / R, qrow = pc % R;
  v8 qf[NKS];
  {
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)qhead * a.hsq + (int64_t)qrow * a.ldq) * 2;
#pragma unroll
    for (int s = 0; s < NKS; ++s)
      qf[s] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (32 * (s >> 1) + 16 * hi + 8 * (s & 1)) * 2));
  }
  uint32_t lim = end;
  if (a.causal) lim = min(lim, qrow + (len > R ? len - R : 0u) + 1u);

  // ---- addresses of a step's two 16-key groups (wave-uniform; BYTE offsets from a.k / a.v: an element is a byte)
  const int64_t khead = (int64_t)kvh * a.hsk, vhead = (int64_t)kvh * a.hsv;
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  auto group_offsets = [&](uint32_t key0, int64_t (&ko)[2], int64_t (&vo)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t key = key0 + 16u * u;
      if (a.paged) {
        // (entries past the sequence's last page are never read)
        const int64_t page = key < end ? (int64_t)a.table[(int64_t)batch * a.tableStride + (key >> a.pageShift)] : 0;
        const int64_t in = (int64_t)(key & pageMask);
        ko[u] = page * a.psk + khead + in * a.ldk;
        vo[u] = page * a.psv + vhead + in * a.ldv;
      } else {
        ko[u] = (int64_t)batch * a.bsk + khead + (int64_t)key * a.ldk;
        vo[u] = (int64_t)batch * a.bsv + vhead + (int64_t)key * a.ldv;
      }
    }
  };

  // K: lane = key row q of the step, bytes 32 u + 16 hi .. + 15 of the row.  V: instruction i covers rows i RPI .. + RPI - 1 whole.
  u32x4 kreg[NKL], vreg[NCH];
  const int vrow0 = lane / CPR, vc = lane % CPR;
  auto issue_loads = [&](uint32_t key0) {
    int64_t ko[2], vo[2];
    group_offsets(key0, ko, vo);
    const bool kvalid = key0 + (uint32_t)q < end;
    const char *kp = a.k + (q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk + 16 * hi;
#pragma unroll
    for (int u = 0; u < NKL; ++u) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + 32 * u);
      kreg[u] = z;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int row = i * RPI + vrow0;
      u32x4 z = {0u, 0u, 0u, 0u};
      if (key0 + (uint32_t)row < end)
        z = *reinterpret_cast<const u32x4 *>(a.v + vo[(i * RPI) >> 4] + (int64_t)(row & 15) * a.ldv + vc * 16);
      vreg[i] = z;
    }
  };

  f32x16 o[NDB];
  float m = DEC_MINUS_HUGE, l = 0.f;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  char *Vs = smem + wave * IMAGE;   // this wave's V image: [D/32][32 keys][32 d], 16-bit
  const int n16 = lane & 15;
  const int vtr_off = ((n16 >> 2) + 4 * hi) * 64 + (((lane >> 4) & 1) * 16 + 4 * (n16 & 3)) * 2;

  uint32_t key0 = begin + (uint32_t)wave * DEC_STEP;
  if (key0 < end) issue_loads(key0);
  while (key0 < end) {
    // ---- S^T = K Q^T: a slice of K is converted at its matrix instruction
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < NKS; ++t) {
      const u32x4 kb = kreg[t >> 1];
      const u32x4 kf = (t & 1) ? cvt8_e4m3<T>(kb[2], kb[3]) : cvt8_e4m3<T>(kb[0], kb[1]);
      s = F::mfma(__builtin_bit_cast(v8, kf), qf[t], s);
    }
    // ---- V rows, converted, to the wave's image: a lane's 16 values of d are the 16-bit chunks 2 vc and 2 vc + 1 of its row
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int row = i * RPI + vrow0;
      char *dst = Vs + ((vc >> 1) * DEC_STEP + row) * 64 + (vc & 1) * 32;
      *reinterpret_cast<u32x4 *>(dst) = cvt8_e4m3<T>(vreg[i][0], vreg[i][1]);
      *reinterpret_cast<u32x4 *>(dst + 16) = cvt8_e4m3<T>(vreg[i][2], vreg[i][3]);
    }
    // ---- the registers are free: the next step's loads fly during the rest of this one
    const uint32_t cur = key0;
    key0 += DEC_WAVES * DEC_STEP;
    if (key0 < end) issue_loads(key0);

    // ---- online softmax over the visible keys only (the K scale rides on the softmax scale)
    float mx = DEC_MINUS_HUGE;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool visible = cur + (uint32_t)crow(r, hi) < lim;
      s[r] = visible ? s[r] * kscale : DEC_MINUS_HUGE;
      mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (mx > m) {
      const float corr = fast_exp2(m - mx);
      m = mx;
      l *= corr;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= corr;
    }
    float psum = 0.f;
    v8 pf[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool visible = cur + (uint32_t)crow(r, hi) < lim;
      const float p = visible ? fast_exp2(s[r] - m) : 0.f;   // replaced, never multiplied
      psum += p;
      pf[r >> 3][r & 7] = (T)p;
    }
    l += psum;

    // ---- O^T += V^T P^T
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const char *vp = Vs + (db * DEC_STEP + 16 * u) * 64 + vtr_off;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vp));
        const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vp + 8 * 64));
        const s16x8 both = __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
        o[db] = F::mfma(__builtin_bit_cast(v8, both), pf[u], o[db]);
      }
  }

  // ---- merge the four waves through LDS (attn_decode16.h); the V scale multiplies what leaves the workgroup
  constexpr int OLD = D + 4;
  float *Om = reinterpret_cast<float *>(smem);                       // [waves][32][OLD]
  float *ms = Om + DEC_WAVES * 32 * OLD, *ls = ms + DEC_WAVES * 32;   // [waves][32] each
  const float l_tot = l + __shfl_xor(l, 32);
  __syncthreads();   // every wave is done with its image
  if (hi == 0) ms[wave * 32 + q] = m;
  __syncthreads();
  float mstar = ms[q];
#pragma unroll
  for (int w = 1; w < DEC_WAVES; ++w) mstar = fmaxf(mstar, ms[w * 32 + q]);
  const float wgt = fast_exp2(m - mstar);   // (all of them -FLT_MAX: 1, on zeros)
  {
    float *orow = Om + (wave * 32 + q) * OLD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)   // crow(4g + i, hi) = i + 8g + 4hi
        *reinterpret_cast<float4 *>(orow + 32 * db + 8 * g + 4 * hi) =
            make_float4(o[db][4 * g] * wgt, o[db][4 * g + 1] * wgt, o[db][4 * g + 2] * wgt, o[db][4 * g + 3] * wgt);
    if (hi == 0) ls[wave * 32 + q] = l_tot * wgt;
  }
  __syncthreads();
  constexpr int CL = D / 4;   // float4 columns per row
  for (int idx = tid; idx < 32 * CL; idx += DEC_WAVES * 64) {
    const uint32_t p = (uint32_t)idx / CL, c = (uint32_t)idx % CL;
    if (p >= M) break;
    float4 acc = *reinterpret_cast<const float4 *>(Om + p * OLD + 4 * c);
    float lsum = ls[p], mrow = ms[p];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
      const float4 x = *reinterpret_cast<const float4 *>(Om + (w * 32 + p) * OLD + 4 * c);
      acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
      lsum += ls[w * 32 + p];
      mrow = fmaxf(mrow, ms[w * 32 + p]);
    }
    const uint32_t head = kvh * a.G + p / R, row = p % R;
    if constexpr (SPLIT) {
      const size_t slab = (((size_t)piece * a.batches + batch) * a.Hq + head) * R + row;
      acc.x *= vscale; acc.y *= vscale; acc.z *= vscale; acc.w *= vscale;
      *reinterpret_cast<float4 *>(a.wsO + slab * D + 4 * c) = acc;
      if (c == 0) *reinterpret_cast<float2 *>(a.wsML + slab * 2) = make_float2(mrow, lsum);
    } else {
      const float inv = lsum > 0.f ? vscale / lsum : 0.f;   // a sequence of length 0: O = 0
      acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
      const int64_t at = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)row * a.ldo + 4 * c;
      if (a.outF32) *reinterpret_cast<float4 *>(a.o + at * 4) = acc;
      else *reinterpret_cast<u32x2 *>(a.o + at * 2) = u32x2{pack16<T>(acc.x, acc.y), pack16<T>(acc.z, acc.w)};
      if (c == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + row] = lsum > 0.f ? mrow + log2f(lsum) : DEC_MINUS_HUGE;
    }
  }
}

} // namespace mfa
